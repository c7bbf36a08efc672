"""The point codec and the subgroup check (zkp_g1/g2_decompress, _compress, _subgroup_check: `decompress_kernel`, `compress_kernel`,
`subgroup_check_kernel` of csrc/msm_group.hip) at their field and grid edges.  tests/test_gpu_codec.py runs 40, 24 and 12 random
multiples of the generator, one 64-lane workgroup; the inputs here come from tests/codec_cases.py (pinned on the CPU by
tests/test_codec_cases.py): Fq2 x with a real x^3 + b (both exits of `curve_sqrt`'s `a.c1 == 0` branch and the c0 tie-break of
`y_positive`), y within one limb of p / 2 for every limb of `fp_gt`, coordinates at and above the modulus in c0 and in c1, the
identity flag beside a non-zero x, x = 0, points of order 3 and cofactor points, and failures in different workgroups and in the
ragged last one with a good call on the same buffers straight after.

The reference in every assertion is oracle/pyref/serialize.py or Python integers, never ckb_zkp_amd/serialize.py and never another
kernel; Montgomery words are compared bit for bit with `codec.g1_to_mont` / `g2_to_mont` of the oracle's point.

Not reached: the lower limbs of `fp_gt` through DEcompress.  No G1 point of either curve has y = (p - 1) / 2, and an on-curve y
within 2^(32 k) of p / 2 would take a cube-root search per limb (codec_cases.no_g1_point_at_half_p); compress reaches them."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec
from ckb_zkp_amd.params import get_curve
from oracle.pyref import serialize as oser
from tests import codec_cases as cc
from tests.util import OC

pytestmark = pytest.mark.gpu
PAIRS = pytest.mark.parametrize("curve,group", cc.PAIRS)
SIZE_MAX = C.c_size_t(-1).value
ZKP_OK = 0                                                       # include/zkp_accel.h zkp_status
XY_SENTINEL, INF_SENTINEL, BYTE_SENTINEL = 0x5A5A5A5A5A5A5A5A, 9, 0xA5


class Env:
    def __init__(self, curve, group):
        self.curve, self.group = curve, group
        self.c, self.oc = get_curve(curve), OC[curve]
        self.pb = 8 * self.c.fq_limbs * group                     # bytes of a compressed point
        self.w = 2 * self.c.fq_limbs * group                      # 64-bit words of an affine point
        self.pool = cc.pool(curve, group)
        self.good_bytes = [oser.point_encode(P, self.oc, group) for P in self.pool]
        self.good_words, _ = self.words(self.pool)
        self.identity = oser.point_encode(None, self.oc, group)

    def words(self, pts):
        """(x, y) integer pairs (on the curve or not) or None -> Montgomery words, identity flags"""
        return (codec.g1_to_mont if self.group == 1 else codec.g2_to_mont)(list(pts), self.c)

    def mont_words(self, mont):
        return codec.ints_to_limbs(mont, self.c.fq_limbs).reshape(-1)

    def fn(self, ctx, name):
        return getattr(ctx.lib, f"zkp_g{self.group}_{name}")


@lru_cache(maxsize=None)
def env(curve, group):
    return Env(curve, group)


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_decompress(ctx, e, data, n, xy, inf):
    buf = np.frombuffer(data, dtype=np.uint8) if data is not None else None
    assert buf is None or len(buf) == n * e.pb
    bad = C.c_size_t(0)
    rc = e.fn(ctx, "decompress")(ctx.h, e.c.cid, _p(buf), n, _p(xy), _p(inf), C.byref(bad))
    return rc, bad.value


def raw_subgroup(ctx, e, xy, inf):
    xy = np.ascontiguousarray(xy, dtype=np.uint64)
    bad = C.c_size_t(0)
    rc = e.fn(ctx, "subgroup_check")(ctx.h, e.c.cid, _p(xy), _p(inf), xy.shape[0], C.byref(bad))
    return rc, bad.value


def raw_compress(ctx, e, xy, inf, n, out):
    return e.fn(ctx, "compress")(ctx.h, e.c.cid, _p(xy), _p(inf), n, _p(out))


def sentinels(e, n):
    return np.full((n, e.w), XY_SENTINEL, dtype=np.uint64), np.full(n, INF_SENTINEL, dtype=np.uint8)


def untouched(xy, inf):
    return bool((xy == XY_SENTINEL).all() and (inf == INF_SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------- decompress
@PAIRS
def test_decompress_accepts_every_valid_edge_encoding(ctx, curve, group):
    """all accepted cases of (a) in ONE call behind 70 pool points: several workgroups, the last one ragged"""
    e = env(curve, group)
    acc = [c for c in cc.decompress_cases(curve, group) if c.want != cc.INVALID]
    lead = 70 if (70 + len(acc)) % 64 else 71
    data = b"".join(e.good_bytes[:lead]) + b"".join(c.data for c in acc)
    n = lead + len(acc)
    assert n > 64 and n % 64
    xy, inf = ctx.decompress_points(e.c, group, data)
    want_xy, want_inf = e.words(list(e.pool[:lead]) + [c.want for c in acc])
    asserted = 0
    for i in range(n):
        name = (curve, group, f"pool {i}" if i < lead else acc[i - lead].name)
        assert int(inf[i]) == int(want_inf[i]), name
        assert np.array_equal(xy[i], want_xy[i]), name                     # the identity: all-zero words
        asserted += 1
    assert sum(c.want is None for c in acc) >= 4 and not xy[[lead + i for i, c in enumerate(acc) if c.want is None]].any()
    print(f"decompress accepted {curve} G{group}: generated {n}, asserted {asserted}")
    assert asserted == n


@PAIRS
def test_decompress_rejects_each_malformed_encoding_with_its_index(ctx, curve, group):
    """each rejected case of (a) on its own at index k of k + 2 good ones (k + 3 points), k cycling through 0, 1, 63, 64, 65; the
    outputs, pre-filled with a sentinel, stay as they were"""
    e = env(curve, group)
    rej = [c for c in cc.decompress_cases(curve, group) if c.want == cc.INVALID]
    assert {c.kind for c in rej} == {"canonical", "noncanonical", "both_flags"}
    asserted = 0
    for j, case in enumerate(rej):
        k = (0, 1, 63, 64, 65)[j % 5]
        data = b"".join(e.good_bytes[:k]) + case.data + b"".join(e.good_bytes[k:k + 2])
        xy, inf = sentinels(e, k + 3)
        rc, bad = raw_decompress(ctx, e, data, k + 3, xy, inf)
        assert (rc, bad) == (_lib.ZKP_ERR_INVALID_POINT, k), (curve, group, case.name, k, rc, bad)
        assert untouched(xy, inf), (curve, group, case.name)
        asserted += 1
    print(f"decompress rejected {curve} G{group}: generated {len(rej)}, asserted {asserted}")
    assert asserted == len(rej)


@PAIRS
def test_decompress_reports_the_first_failure_of_any_workgroup_and_recovers(ctx, curve, group):
    e = env(curve, group)
    rej = [c for c in cc.decompress_cases(curve, group) if c.want == cc.INVALID]
    lays = cc.failure_layouts()
    asserted = used = 0
    for lay in lays:
        enc = list(e.good_bytes[:lay.n])
        for b in lay.bad:
            enc[b] = rej[used % len(rej)].data
            used += 1
        xy, inf = sentinels(e, lay.n)
        rc, bad = raw_decompress(ctx, e, b"".join(enc), lay.n, xy, inf)
        assert (rc, bad) == (_lib.ZKP_ERR_INVALID_POINT, lay.first), (curve, group, lay, rc, bad)
        assert untouched(xy, inf), (curve, group, lay)
        # the same buffers, good points only: a status word that is not re-armed would fail this call
        rc, bad = raw_decompress(ctx, e, b"".join(e.good_bytes[:lay.n]), lay.n, xy, inf)
        assert (rc, bad) == (ZKP_OK, SIZE_MAX), (curve, group, lay, rc, bad)
        assert np.array_equal(xy, e.good_words[:lay.n]) and not inf.any(), (curve, group, lay)
        asserted += 1
    print(f"decompress layouts {curve} G{group}: generated {len(lays)}, asserted {asserted}")
    assert asserted == len(lays)


# --------------------------------------------------------------------------------------------------------------- compress
@PAIRS
def test_compress_matches_point_encode_on_every_sign_edge_and_identity_rule(ctx, curve, group):
    """all of (b).  The y values are off the curve: neither `compress_kernel` nor `oser.point_encode` tests the curve equation"""
    e = env(curve, group)
    cases = cc.compress_cases(curve, group)
    asserted = 0
    for with_inf in (True, False):
        part = [c for c in cases if (c.inf is not None) == with_inf]
        xy, _ = e.words([(c.x, c.y) for c in part])
        inf = np.array([c.inf for c in part], dtype=np.uint8) if with_inf else None
        got = ctx.compress_points(e.c, group, xy, inf)
        assert len(got) == len(part) * e.pb and len(part) > (64 if with_inf else 1)
        for i, c in enumerate(part):
            assert got[i * e.pb:(i + 1) * e.pb] == c.want, (curve, group, c.name)
            asserted += 1
    print(f"compress edges {curve} G{group}: generated {len(cases)}, asserted {asserted}")
    assert asserted == len(cases)


@PAIRS
def test_accepted_edge_points_round_trip(ctx, curve, group):
    """every on-curve point that (a) produced: compress gives the bytes it was decoded from, decompress gives the words back"""
    e = env(curve, group)
    acc = [c for c in cc.decompress_cases(curve, group) if c.want not in (None, cc.INVALID)]
    xy, inf = e.words([c.want for c in acc])
    got = ctx.compress_points(e.c, group, xy, inf)
    asserted = 0
    for i, c in enumerate(acc):
        assert got[i * e.pb:(i + 1) * e.pb] == c.data == oser.point_encode(c.want, e.oc, group), (curve, group, c.name)
        asserted += 1
    xy2, inf2 = ctx.decompress_points(e.c, group, got)
    differ = [acc[i].name for i in range(len(acc)) if not np.array_equal(xy2[i], xy[i]) or inf2[i]]
    assert not differ, (curve, group, differ[:4])
    print(f"round trips {curve} G{group}: generated {len(acc)}, asserted {asserted}")
    assert asserted == len(acc)


@PAIRS
def test_compress_sizes_around_the_workgroup_keep_the_bytes_behind_the_last_point(ctx, curve, group):
    e = env(curve, group)
    special = [c for c in cc.compress_cases(curve, group) if c.inf is not None]
    sizes = (1, 63, 64, 65, 129)
    asserted = 0
    for n in sizes:
        pts, flags, want = [], [], []
        for i in range(n):
            if i % 7 == 3:
                pts.append(None), flags.append(1), want.append(e.identity)
            elif i % 5 == 1:
                c = special[(n + 11 * i) % len(special)]
                pts.append((c.x, c.y)), flags.append(c.inf), want.append(c.want)
            else:
                pts.append(e.pool[(n + i) % cc.POOL]), flags.append(0), want.append(e.good_bytes[(n + i) % cc.POOL])
        xy, _ = e.words(pts)
        out = np.full(n * e.pb + 64, BYTE_SENTINEL, dtype=np.uint8)
        rc = raw_compress(ctx, e, xy, np.array(flags, dtype=np.uint8), n, out)
        assert rc == ZKP_OK
        assert out[:n * e.pb].tobytes() == b"".join(want), (curve, group, n)
        assert (out[n * e.pb:] == BYTE_SENTINEL).all(), (curve, group, n)
        asserted += 1
    print(f"compress sizes {curve} G{group}: generated {len(sizes)}, asserted {asserted}")
    assert asserted == len(sizes)


# --------------------------------------------------------------------------------------------------------- subgroup check
def _sub_row(e, case):
    return e.mont_words(case.mont)


@PAIRS
def test_subgroup_check_gives_the_oracle_verdict_on_every_case(ctx, curve, group):
    """every case of (c) alone at index 66 of 71 points (the second workgroup), then all rejected ones in one call.  BN254 G1 has
    cofactor 1: no curve point lies outside its subgroup, so its list holds the off-curve and skipped-lane cases only."""
    e = env(curve, group)
    cases = cc.subgroup_cases(curve, group)
    asserted = 0
    for case in cases:
        xy = e.good_words[:71].copy()
        xy[66] = _sub_row(e, case)
        inf = None
        if case.inf is not None:
            inf = np.zeros(71, dtype=np.uint8)
            inf[66] = case.inf
        rc, bad = raw_subgroup(ctx, e, xy, inf)
        want = (ZKP_OK, SIZE_MAX) if case.want else (_lib.ZKP_ERR_INVALID_POINT, 66)
        assert (rc, bad) == want, (curve, group, case.name, rc, bad)
        asserted += 1
    rej = [c for c in cases if not c.want]
    assert len(rej) >= 2 and ((curve, group) == ("bn254", 1) or any(c.kind == "cofactor" for c in rej))
    n = 150
    pos = [(140 - 37 * j) % n for j in range(len(rej))]                       # 140, 103, 66, 29, 142, ...: not in index order
    assert len(set(pos)) == len(pos) and pos[0] != min(pos)
    xy = e.good_words[:n].copy()
    for k, case in zip(pos, rej):
        xy[k] = _sub_row(e, case)
    rc, bad = raw_subgroup(ctx, e, xy, np.zeros(n, dtype=np.uint8))
    assert (rc, bad) == (_lib.ZKP_ERR_INVALID_POINT, min(pos)), (curve, group, rc, bad, sorted(pos))
    asserted += 1
    with pytest.raises(ValueError) as err:                                     # and through the Python entry
        ctx.subgroup_check(e.c, group, xy, np.zeros(n, dtype=np.uint8))
    assert f"point {min(pos)} " in str(err.value)
    print(f"subgroup cases {curve} G{group}: generated {len(cases) + 1}, asserted {asserted}")
    assert asserted == len(cases) + 1


@PAIRS
def test_subgroup_check_reports_the_first_failure_of_any_workgroup_and_recovers(ctx, curve, group):
    """off-curve points and curve points outside the subgroup as the bad ones, in separate layouts (BN254 G1: off-curve only, see
    above)"""
    e = env(curve, group)
    cases = cc.subgroup_cases(curve, group)
    kinds = {"off_curve": [c for c in cases if c.kind == "off_curve"],
             "outside": [c for c in cases if c.kind in ("low_order", "cofactor")]}
    assert kinds["off_curve"] and (bool(kinds["outside"]) == ((curve, group) != ("bn254", 1)))
    lays = cc.failure_layouts()
    asserted = generated = 0
    for kind, bads in kinds.items():
        for lay in (lays if bads else ()):
            generated += 1
            xy = e.good_words[:lay.n].copy()
            inf = np.zeros(lay.n, dtype=np.uint8)
            for j, b in enumerate(lay.bad):
                xy[b] = _sub_row(e, bads[(j + lay.n) % len(bads)])
            rc, bad = raw_subgroup(ctx, e, xy, inf)
            assert (rc, bad) == (_lib.ZKP_ERR_INVALID_POINT, lay.first), (curve, group, kind, lay, rc, bad)
            rc, bad = raw_subgroup(ctx, e, e.good_words[:lay.n], inf)           # re-armed: the good points pass straight after
            assert (rc, bad) == (ZKP_OK, SIZE_MAX), (curve, group, kind, lay, rc, bad)
            asserted += 1
    print(f"subgroup layouts {curve} G{group}: generated {generated}, asserted {asserted}")
    assert asserted == generated == len(lays) * (1 + bool(kinds["outside"]))


# ------------------------------------------------------------------------------------------------------------------ n == 0
@PAIRS
def test_zero_points_succeed_and_write_nothing(ctx, curve, group):
    e = env(curve, group)
    asserted = 0
    xy, inf = sentinels(e, 2)
    data = np.full(2 * e.pb, BYTE_SENTINEL, dtype=np.uint8)
    for null in (True, False):
        bad = C.c_size_t(5)
        rc = e.fn(ctx, "decompress")(ctx.h, e.c.cid, None if null else _p(data), 0, None if null else _p(xy),
                                     None if null else _p(inf), C.byref(bad))
        assert (rc, bad.value) == (ZKP_OK, SIZE_MAX), (curve, group, null, rc, bad.value)
        rc = e.fn(ctx, "compress")(ctx.h, e.c.cid, None if null else _p(xy), None if null else _p(inf), 0, None if null else _p(data))
        assert rc == ZKP_OK, (curve, group, null, rc)
        assert untouched(xy, inf) and (data == BYTE_SENTINEL).all()
        asserted += 2
    assert ctx.compress_points(e.c, group, np.zeros((0, e.w), dtype=np.uint64), np.zeros(0, dtype=np.uint8)) == b""
    got_xy, got_inf = ctx.decompress_points(e.c, group, b"")
    assert got_xy.shape == (0, e.w) and got_inf.shape == (0,)
    asserted += 2
    print(f"n = 0 {curve} G{group}: generated 6, asserted {asserted}")
    assert asserted == 6
