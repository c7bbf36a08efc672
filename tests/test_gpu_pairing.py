"""zkp_pairing_* on the device, both curves, bit for bit against Python integers (tests/pairing_ref.py).

Expected values come from ONE oracle pairing per curve per session, E = e(G1, G2), by bilinearity: for P = [a] G1 and Q = [b] G2 the
device returns E^(s k a b), k = GT_POWER and s the oracle's sign (pairing_ref.py).  Points are made on the device
(zkp_fixed_base_mul_*), outputs are framed by sentinel rows and compared word for word.

Shapes (n, group): (1, 1) one lane; (4, 4); (130, 2) two workgroups plus one group; (65, 65) one wave plus one lane: a group in two
workgroups; (260, 65) groups that straddle workgroup boundaries at different offsets; (257, 257) a group of five workgroups; and
(128, 64), beyond the issue's list: the largest group that still divides a workgroup.  A group size that divides 64 takes the
one-stage path (the heads write the output: (1, 1), (4, 4), (130, 2), (128, 64)), every other the second stage (the 65s, 257, and
the groups of 5 of the identity test).  Every
group's scalars satisfy sum a_i b_i = 0 mod r, so its product is 1; one designated group per shape is off by one in a single scalar
and must give E^(s k b_0) and ok = 0."""
import functools
import random

import numpy as np
import pytest

from ckb_zkp_amd import codec
from ckb_zkp_amd import pairing as zp
from ckb_zkp_amd.params import get_curve
from oracle.pyref.pairing import Fp12
from tests import pairing_ref as ref

pytestmark = pytest.mark.gpu
CURVES = list(ref.CURVE_NAMES)
SENT = 0xDEADBEEFCAFEF00D
SENT_FLAG = 0xA5
SHAPES = [(1, 1), (4, 4), (130, 2), (65, 65), (260, 65), (257, 257), (128, 64)]


class Framed:
    """a device buffer of rows between two sentinel rows"""

    def __init__(self, ctx, rows: np.ndarray, sentinel):
        self.ctx = ctx
        frame = np.full((1,) + rows.shape[1:], sentinel, dtype=rows.dtype)
        self.host = np.concatenate([frame, rows, frame])
        self.dev = ctx.to_device(self.host)
        self.ptr = self.dev + self.host[0].nbytes

    def read(self):
        got = np.zeros_like(self.host)
        self.ctx.d2h(got, self.dev)
        assert np.array_equal(got[0], self.host[0]) and np.array_equal(got[-1], self.host[-1]), "a write outside the buffer"
        return got[1:-1]

    def unchanged(self):
        return np.array_equal(self.read(), self.host[1:-1])

    def free(self):
        self.ctx.dev_free(self.dev)


def device_points(ctx, c, a_list, b_list):
    """([a] G1, [b] G2) as Montgomery words and flags, through zkp_fixed_base_mul_*"""
    g1, i1 = ctx.fixed_base_mul(c, 1, codec.g1_to_mont([c.g1], c)[0], codec.fr_canonical(a_list, c))
    g2, i2 = ctx.fixed_base_mul(c, 2, codec.g2_to_mont([c.g2], c)[0], codec.fr_canonical(b_list, c))
    return g1, i1, g2, i2


def gt_words(curve, flat):
    return zp.fq12_to_mont(flat, get_curve(curve))


class Run:
    """n pairs in framed device buffers"""

    def __init__(self, ctx, c, g1, i1, g2, i2):
        self.ctx, self.c, self.n = ctx, c, len(g1)
        self.b = [Framed(ctx, np.ascontiguousarray(g1), SENT), Framed(ctx, np.ascontiguousarray(i1, dtype=np.uint8), SENT_FLAG),
                  Framed(ctx, np.ascontiguousarray(g2), SENT), Framed(ctx, np.ascontiguousarray(i2, dtype=np.uint8), SENT_FLAG)]
        self.extra = []

    def out(self, rows, words=None, flag=False):
        if flag:
            f = Framed(self.ctx, np.full(rows, SENT_FLAG, dtype=np.uint8), SENT_FLAG)
        else:
            f = Framed(self.ctx, np.full((rows, words), SENT, dtype=np.uint64), SENT)
        self.extra.append(f)
        return f

    def ptrs(self):
        return [x.ptr for x in self.b]

    def inputs_unchanged(self):
        return all(x.unchanged() for x in self.b)

    def free(self):
        for x in self.b + self.extra:
            x.free()


def gt_of_groups(ctx, c, run, group):
    """miller + final_exp (out of place) -> (m, words); also checks that product_is_one agrees with the GT values"""
    m = run.n // group
    w = 12 * c.fq_limbs
    f, gt, ok = run.out(m, w), run.out(m, w), run.out(m, flag=True)
    ctx.pairing_miller_dev(c, *run.ptrs(), run.n, group, f.ptr)
    ctx.pairing_final_exp_dev(c, f.ptr, m, gt.ptr)
    ctx.pairing_product_is_one_dev(c, *run.ptrs(), run.n, group, ok.ptr)
    got, flags = gt.read(), ok.read()
    assert run.inputs_unchanged(), "an input changed"
    one = gt_words(c.name, zp.gt_one())
    assert [int(x) for x in flags] == [1 if np.array_equal(row, one) else 0 for row in got]
    return got, flags


# ------------------------------------------------------------------------------------------- the pairing value
@pytest.mark.parametrize("curve", CURVES)
def test_pairing_value(ctx, curve):
    c = get_curve(curve)
    rng = random.Random(f"pairing-{curve}")
    r = c.r
    top = 1 << (r.bit_length() - 1)
    ab = [(1, 1), (1, r - 1), (r - 1, 1), (2, 3), (rng.randrange(top, r), rng.randrange(top, r))]      # full-length scalars
    g1, i1, g2, i2 = device_points(ctx, c, [a for a, _ in ab], [b for _, b in ab])
    assert codec.g1_from_mont(g1[:1], None, c)[0] == c.g1                # the generator itself: BN254's (1, 2)
    got = ctx.pairing(c, g1, i1, g2, i2)
    for k, (a, b) in enumerate(ab):
        assert np.array_equal(got[k], gt_words(curve, ref.expected_pairing(curve, a, b))), (a, b)
    assert zp.pairing(ctx, c, c.g1, c.g2) == ref.expected_pairing(curve, 1, 1)
    assert ctx.pairing_info(c)["gt_power"] == zp.GT_POWER[curve] == ref.GT_POWER[curve]
    assert ctx.pairing_info(c)["fq12_words"] == 12 * c.fq_limbs and ctx.pairing_info(c)["pairs_per_workgroup"] == 64


# ------------------------------------------------------------------------------------------- groups and product trees
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("curve", CURVES)
def test_groups(ctx, curve, shape):
    c = get_curve(curve)
    n, group = shape
    m = n // group
    rng = random.Random(f"groups-{curve}-{n}-{group}")
    one = zp.gt_one()
    # the group that is off by one; a shape of one group runs twice, so that its only group is seen giving 1 as well
    for off in ([None, 0] if m == 1 else [m // 2]):
        pairs, want = [], []
        for j in range(m):
            grp = ref.balanced_group(curve, group, rng, off_by_one=(j == off))
            pairs += grp
            want.append(ref.expected_product(curve, grp))
        assert all((w == one) == (j != off) for j, w in enumerate(want))
        g1, i1, g2, i2 = device_points(ctx, c, [a for a, _ in pairs], [b for _, b in pairs])
        run = Run(ctx, c, g1, i1, g2, i2)
        try:
            got, flags = gt_of_groups(ctx, c, run, group)
        finally:
            run.free()
        for j in range(m):
            assert np.array_equal(got[j], gt_words(curve, want[j])), (shape, off, j)
        assert [int(x) for x in flags] == [0 if j == off else 1 for j in range(m)]
        assert list(ctx.pairing_check(c, g1, i1, g2, i2, group)) == [0 if j == off else 1 for j in range(m)]      # the host entry


# ------------------------------------------------------------------------------------------- identities
@pytest.mark.parametrize("curve", CURVES)
def test_identities(ctx, curve):
    c = get_curve(curve)
    rng = random.Random(f"identities-{curve}")
    group = 5
    # group 0: flagged G1 first, flagged G2 last; group 1: both flagged at once in the middle; group 2: only identities;
    # group 3: nothing flagged
    ab = [(rng.randrange(1, c.r), rng.randrange(1, c.r)) for _ in range(4 * group)]
    g1, i1, g2, i2 = device_points(ctx, c, [a for a, _ in ab], [b for _, b in ab])
    live = [True] * len(ab)
    for k, (f1, f2) in {0: (1, 0), 4: (0, 1), 7: (1, 1), 10: (1, 0), 11: (0, 1), 12: (1, 1), 13: (1, 0), 14: (0, 1)}.items():
        i1[k], i2[k] = f1, f2                                            # the words stay those of real points
        live[k] = False
    want = [ref.expected_product(curve, [p for k, p in enumerate(ab) if live[k] and k // group == j]) for j in range(4)]
    assert want[2] == zp.gt_one()
    run = Run(ctx, c, g1, i1, g2, i2)
    try:
        got, flags = gt_of_groups(ctx, c, run, group)
    finally:
        run.free()
    for j in range(4):
        assert np.array_equal(got[j], gt_words(curve, want[j])), j
    assert [int(x) for x in flags] == [0, 0, 1, 0]
    # one pair per lane, group 1: a flagged pair alone gives one
    assert np.array_equal(ctx.pairing(c, g1[:1], i1[:1], g2[:1], i2[:1])[0], gt_words(curve, zp.gt_one()))


# ------------------------------------------------------------------------------------------- the Miller kernel alone
@pytest.mark.parametrize("curve", CURVES)
def test_miller_alone(ctx, curve):
    """three pairs in one group; the raw value is defined only up to factors that the final exponentiation removes, so it is raised
    by the oracle's exponent and compared with the oracle's own product (2 oracle powers)"""
    c = get_curve(curve)
    oc = ref.curve(curve)
    F, pr = Fp12(oc), ref.pairing(curve)
    ab = [(3, 5), (7, 2), (oc.r - 4, 6)]
    pts1, pts2 = [ref.g1_mul(curve, a) for a, _ in ab], [ref.g2_mul(curve, b) for _, b in ab]
    (f,) = zp.miller_products(ctx, c, pts1, pts2, 3)
    prod = F.one
    for P, Q in zip(pts1, pts2):
        prod = F.mul(prod, pr.miller(P, Q))
    want = F.pow(prod, pr.final_exp)
    if curve == "bls12_381":                                             # the oracle does not conjugate: it holds e^-1 there
        want = F.pow(want, oc.r - 1)
    assert F.pow(f, pr.final_exp) == want
    assert want == ref.gt_pow(curve, ref.sign(curve) * sum(a * b for a, b in ab))


# ------------------------------------------------------------------------------------------- the final exponentiation alone
@functools.lru_cache(maxsize=None)
def _random_and_its_power(curve):
    """a random Fq12 (not a Miller value) and F12.pow(f, k final_exp): the one oracle power of the final-exponentiation tests"""
    oc = ref.curve(curve)
    rng = random.Random(f"final-exp-{curve}")
    f = [(rng.randrange(oc.q), rng.randrange(oc.q)) for _ in range(6)]
    return f, Fp12(oc).pow(f, ref.GT_POWER[curve] * ((oc.q ** 12 - 1) // oc.r))


@pytest.mark.parametrize("m", [1, 65])
@pytest.mark.parametrize("curve", CURVES)
def test_final_exp_alone(ctx, curve, m):
    c = get_curve(curve)
    oc = ref.curve(curve)
    F, T = Fp12(oc), ref.tower(curve)
    rand, want_rand = _random_and_its_power(curve)
    rng = random.Random(f"final-exp-{curve}-{m}")
    zero = [(0, 0)] * 6
    fs, want = [rand], [want_rand]
    if m > 1:
        fs += [zp.gt_one(), [(rng.randrange(1, c.q), 0)] + [(0, 0)] * 5, zero]          # 1, an element of Fq, 0
        want += [zp.gt_one(), zp.gt_one(), zero]
    while len(fs) < m:                                                   # further random elements: the chain's model (test_pairing_ref.py)
        x = T.random(rng)
        fs.append(T.to_flat(x))
        want.append(T.to_flat(T.final_exp(x)))
    rows = np.stack([zp.fq12_to_mont(f, c) for f in fs])
    src = Framed(ctx, rows, SENT)
    dst = Framed(ctx, np.full_like(rows, SENT), SENT)
    try:
        ctx.pairing_final_exp_dev(c, src.ptr, len(fs), dst.ptr)
        got = dst.read()
        assert src.unchanged()
        ctx.pairing_final_exp_dev(c, src.ptr, len(fs), src.ptr)          # in place
        assert np.array_equal(src.read(), got)
    finally:
        src.free()
        dst.free()
    for k, w in enumerate(want):
        assert np.array_equal(got[k], gt_words(curve, w)), k
    for k in range(len(fs)):
        if fs[k] != zero:
            assert F.pow(zp.fq12_from_mont(got[k], c), oc.r) == F.one    # in GT
    assert zp.final_exponentiation(ctx, c, fs[:4]) == want[:4]


# ------------------------------------------------------------------------------------------- argument rules
@pytest.mark.parametrize("curve", CURVES)
def test_argument_rules(ctx, curve):
    c = get_curve(curve)
    n, group = 6, 3
    w = 12 * c.fq_limbs
    g1, i1, g2, i2 = device_points(ctx, c, list(range(1, n + 1)), list(range(2, n + 2)))
    run = Run(ctx, c, g1, i1, g2, i2)
    f = run.out(n, w)
    ok = run.out(n, flag=True)
    p1, q1, p2, q2 = run.ptrs()
    lib, h = ctx.lib, ctx.h
    import ctypes as C
    vp = C.c_void_p

    def miller(a=p1, b=q1, cc=p2, d=q2, nn=n, g=group, o=None, cid=c.cid):
        return lib.zkp_pairing_miller_dev(h, cid, vp(a), vp(b), vp(cc), vp(d), nn, g, vp(f.ptr if o is None else o))

    def is_one(a=p1, b=q1, cc=p2, d=q2, nn=n, g=group, o=None, cid=c.cid):
        return lib.zkp_pairing_product_is_one_dev(h, cid, vp(a), vp(b), vp(cc), vp(d), nn, g, vp(ok.ptr if o is None else o))

    def fexp(a=None, mm=2, o=None, cid=c.cid):
        return lib.zkp_pairing_final_exp_dev(h, cid, vp(f.ptr if a is None else a), mm, vp(f.ptr if o is None else o))

    try:
        for fn in (miller, is_one):
            assert fn() == 0                                             # the baseline is accepted
        f.host[1:-1] = f.read()                                          # what the accepted calls left is the new reference
        ok.host[1:-1] = ok.read()
        bad = []
        for fn in (miller, is_one):
            bad += [fn(a=0), fn(b=0), fn(cc=0), fn(d=0), fn(o=0)]                       # NULL pointers
            bad += [fn(a=p1 + 8), fn(cc=p2 + 8)]                                         # misaligned points
            bad += [fn(nn=0), fn(g=0), fn(nn=0, g=0), fn(g=4), fn(nn=5, g=3)]            # empty, not a multiple
            bad += [fn(nn=(1 << 20) + 1, g=1), fn(nn=1 << 21, g=2)]                      # above the cap
            bad += [fn(cid=2), fn(cid=-1)]                                               # unknown curve
        bad += [miller(o=f.ptr + 8)]                                                     # misaligned Fq12
        bad += [miller(o=p1), miller(o=p2), miller(o=p2 + 64), is_one(o=q1), is_one(o=q2), is_one(o=p1 + 16)]   # output over an input
        bad += [fexp(a=0), fexp(o=0), fexp(mm=0), fexp(mm=(1 << 20) + 1), fexp(cid=7)]
        bad += [fexp(a=f.ptr + 8), fexp(o=f.ptr + 8)]                                    # misaligned
        bad += [fexp(a=f.ptr, o=f.ptr + 8 * w), fexp(a=f.ptr + 8 * w, o=f.ptr)]          # partial overlap; in place is allowed
        assert bad == [-1] * len(bad), bad
        ctx.sync()
        assert f.unchanged() and ok.unchanged() and run.inputs_unchanged(), "a refused call wrote"
        # the host entries
        gt = np.full((n, w), SENT, dtype=np.uint64)
        okh = np.full(n // group, SENT_FLAG, dtype=np.uint8)
        A = lambda a: vp(a.ctypes.data)
        hb = []
        hb += [lib.zkp_pairing(h, c.cid, None, A(i1), A(g2), A(i2), n, A(gt)), lib.zkp_pairing(h, c.cid, A(g1), A(i1), A(g2), A(i2), n, None)]
        hb += [lib.zkp_pairing(h, c.cid, A(g1), A(i1), A(g2), A(i2), 0, A(gt)), lib.zkp_pairing(h, 5, A(g1), A(i1), A(g2), A(i2), n, A(gt))]
        hb += [lib.zkp_pairing(h, c.cid, A(g1), A(i1), A(g2), A(i2), (1 << 20) + 1, A(gt))]
        hb += [lib.zkp_pairing_check(h, c.cid, A(g1), A(i1), A(g2), None, n, group, A(okh)),
               lib.zkp_pairing_check(h, c.cid, A(g1), A(i1), A(g2), A(i2), n, 4, A(okh)),
               lib.zkp_pairing_check(h, c.cid, A(g1), A(i1), A(g2), A(i2), n, 0, A(okh)),
               lib.zkp_pairing_check(h, c.cid, A(g1), A(i1), A(g2), A(i2), n, group, A(i1))]
        assert hb == [-1] * len(hb), hb
        assert (gt == SENT).all() and (okh == SENT_FLAG).all()
        info = (C.c_uint64 * 8)()
        assert lib.zkp_pairing_info(3, info) == -1 and lib.zkp_pairing_info(c.cid, None) == -1
    finally:
        run.free()
