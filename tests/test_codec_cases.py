"""tests/codec_cases.py pinned without a GPU: the generator's own claims (counts per kind, the zero-imaginary-part search, the sign
ties, the order-3 point) and the product's HOST codec (ckb_zkp_amd/serialize.py) against the oracle's verdict on every case.
`serialize._sqrt_fq2` is the same norm method as the kernel's `curve_sqrt(Fp2)`, the oracle uses the one-chain complex method:
a disagreement here is the cheap early warning for tests/test_gpu_codec_edges.py."""
import pytest

from ckb_zkp_amd import serialize
from oracle.pyref import serialize as oser
from oracle.pyref.curves import Group
from tests import codec_cases as cc
from tests.util import OC

PAIRS = pytest.mark.parametrize("curve,group", cc.PAIRS)


@PAIRS
def test_case_lists_meet_their_minimums(curve, group):
    oc = OC[curve]
    p, G = oc.q, Group(oc, group)
    dec, comp, sub = cc.decompress_cases(curve, group), cc.compress_cases(curve, group), cc.subgroup_cases(curve, group)
    print(f"{curve} G{group}: decompress {len(dec)} {cc.counts(dec)}; compress {len(comp)} {cc.counts(comp)}; "
          f"subgroup {len(sub)} {cc.counts(sub)}; layouts {len(cc.failure_layouts())}")
    for cases in (dec, comp, sub):
        names = [c.name for c in cases]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    # (a) every canonical x with both y flags; both verdicts occur; accepted points are on the curve with the asked-for sign
    can = [c for c in dec if c.kind == "canonical"]
    nx = len(cc.field_edges(curve))
    assert len(can) == (2 * nx if group == 1 else 2 * (6 * nx - 9))                  # G2: 3 x 3 pairs of {0, 1, p-1} come up twice
    assert any(c.want == cc.INVALID for c in can) and any(c.want not in (None, cc.INVALID) for c in can)
    for c in dec:
        if c.want not in (None, cc.INVALID):
            assert G.on_curve(c.want), c.name
            assert oser.point_encode(c.want, oc, group) == c.data, c.name              # round trip, flag included
    zero_x = [c for c in can if c.data[:-1] == bytes(len(c.data) - 1) and c.data[-1] & 0x3F == 0]
    assert len(zero_x) == 2
    if (curve, group) == ("bls12_381", 1):                                           # x = 0 is the curve point (0, +-2) there only
        assert sorted(c.want for c in zero_x) == [(0, 2), (0, p - 2)]
    else:
        assert all(c.want == cc.INVALID for c in zero_x)
    kinds = cc.counts(dec)
    assert kinds["identity"] == (4 if group == 1 else 10) and kinds["both_flags"] == 2
    nbad = 3 if curve == "bn254" else 4                                              # BLS12-381: 2^381 too; 2^382 - 1 IS all-ones there
    assert kinds["noncanonical"] == (3 * nbad if group == 1 else 3 * (2 * nbad + 1))
    if group == 2:
        zs = cc.zero_imaginary_xs(curve)
        for kind in ("real", "imag"):
            c1s = {c1 for c1, _, k, _ in zs if k == kind}
            assert len(c1s) >= 4, (curve, kind, c1s)
            assert kinds[f"zero_im_{kind}"] == 2 * sum(1 for z in zs if z[2] == kind) >= 8
        for c1, x, _, _ in zs:
            assert (p - x[0], c1) in [z[1] for z in zs]                             # both signs of c0
        print(f"{curve} G2 zero imaginary part: c1 real {sorted({z[0] for z in zs if z[2] == 'real'})}, "
              f"imag {sorted({z[0] for z in zs if z[2] == 'imag'})}")
    # (b) sign ties: exactly one of {y, -y} carries the flag, in Fq and on the c0 tie-break of Fq2
    ny = len(cc.y_edges(curve))
    assert ny == 6 + 2 * cc.limbs32(curve)
    flag = {(c.x, c.y): c.want[-1] & cc.POS for c in comp if c.kind in ("y_edge", "y_tie")}
    assert len(flag) == (4 * ny if group == 1 else 3 * 4 * ny)
    for (x, y), f in flag.items():
        v = y if group == 1 else (y[1] or y[0])                                      # the coordinate that decides
        assert f == (cc.POS if v > p - v else 0), (curve, group, x, y)
        if group == 1 or y[1] == 0 or y[0] == 0:                                      # -y is a case too
            assert flag[(x, G.F.neg(y))] == cc.POS - f, (curve, group, x, y)
    assert kinds_ok(cc.counts(comp), group, ny)
    # (c)
    ksub = cc.counts(sub)
    assert ksub["control"] == 1 and ksub["skipped"] == 4 and ksub["off_curve"] == (2 if group == 1 else 4)
    assert ksub.get("cofactor", 0) == (0 if (curve, group) == ("bn254", 1) else 3)
    assert ksub.get("low_order", 0) == (4 if (curve, group) == ("bls12_381", 1) else 0)
    assert all(c.want == (c.kind in ("control", "skipped")) for c in sub)
    assert cc.no_g1_point_at_half_p(curve)


def kinds_ok(k, group, ny):
    return k["identity_rule"] == 5 and k["y_edge"] == (4 * ny if group == 1 else 9 * ny) and k.get("y_tie", 0) == (0 if group == 1 else 3 * ny)


def test_y_edge_flags_are_0_2_0_2():
    """the issue's spot values: y in {1, p-1, (p-1)/2, (p+1)/2} -> flags 0, 2, 0, 2 (bit 7 of the last byte) on both curves, and the
    same for (y, 0) in Fq2"""
    for curve in cc.CURVES:
        p = OC[curve].q
        for y, want in ((1, 0), (p - 1, cc.POS), ((p - 1) // 2, 0), ((p + 1) // 2, cc.POS)):
            assert oser.point_encode((1, y), OC[curve], 1)[-1] & 0xC0 == want
            assert oser.point_encode(((1, 0), (y, 0)), OC[curve], 2)[-1] & 0xC0 == want
            assert oser.point_encode(((1, 0), (7, y)), OC[curve], 2)[-1] & 0xC0 == want


def test_failure_layouts():
    lay = cc.failure_layouts()
    assert len(lay) == len(set(lay)) == 20
    assert all(l.first == min(l.bad) and max(l.bad) < l.n for l in lay)
    assert {l.n for l in lay} == {1, 63, 64, 65, 128, 129, 193}
    assert cc.Layout(193, (192, 65, 130), 65) in lay and cc.Layout(129, (128, 65), 65) in lay and cc.Layout(65, (64, 63), 63) in lay
    assert not any(l.bad == (192, 65, 130) for l in lay if l.n < 193)


@PAIRS
def test_host_codec_gives_the_oracle_verdict(curve, group):
    oc = OC[curve]
    G = Group(oc, group)
    from_b = serialize.g1_from_bytes if group == 1 else serialize.g2_from_bytes
    to_b = serialize.g1_to_bytes if group == 1 else serialize.g2_to_bytes
    asserted = 0
    dec = cc.decompress_cases(curve, group)
    for c in dec:
        try:
            got = from_b(c.data, curve, checked=False)
        except serialize.SerializationError:
            got = cc.INVALID
        assert got == c.want, (curve, group, c.name)
        asserted += 1
    # neither to_bytes tests the curve equation: all of (b) goes through it; the identity rules are the ABI's (a flag array
    # beside the words), the host codec has None for every one of them
    comp = cc.compress_cases(curve, group)
    for c in comp:
        P = None if c.want == oser.point_encode(None, oc, group) else (c.x, c.y)
        assert to_b(P, curve) == c.want, (curve, group, c.name)
        asserted += 1
    # `in_prime_order_subgroup` assumes a curve point, as ark's: the off-curve cases are left to the kernel's test
    sub = [c for c in cc.subgroup_cases(curve, group) if c.kind in ("control", "low_order", "cofactor")]
    for c in sub:
        P = cc.from_mont(curve, c.mont)
        assert G.on_curve(P) and serialize.in_prime_order_subgroup(P, curve, group) == c.want, (curve, group, c.name)
        asserted += 1
    print(f"host codec {curve} G{group}: generated {len(dec) + len(comp) + len(sub)}, asserted {asserted}")
    assert asserted == len(dec) + len(comp) + len(sub)


@PAIRS
def test_pool_is_in_the_subgroup(curve, group):
    pts = cc.pool(curve, group)
    assert len(pts) == cc.POOL
    for P in (pts[0], pts[17], pts[-1]):
        assert oser.in_subgroup(P, OC[curve], group)
