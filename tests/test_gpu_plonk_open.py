"""zkp_fr_poly_eval_many_dev / zkp_fr_lincomb_dev and rounds 4-5 of ckb_zkp_amd.plonk on the device, bit-exact against Python
integers (tests/plonk_open_ref.py for the driver).  Every output starts as sentinels with one sentinel element before and after
it, whole buffers are compared, and the inputs are read back and compared after the calls."""
import ctypes

import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec, kzg10, plonk
from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.plonk import FR_OPEN_EVAL_GROUP, FR_OPEN_EVAL_MAX_BLOCKS, FR_OPEN_EVAL_THREADS, FR_OPEN_MAX_POLYS
from oracle.pyref.curves import Group
from tests import plonk_open_ref as oref
from tests import plonk_ref as ref
from tests.plonk_cases import KS, MINI_CHALLENGES, challenges, mini_circuit, rand_fr, random_circuit
from tests.util import OC

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xABABABABABABABAB
BAD_ARG = -1
TMAX = FR_OPEN_EVAL_THREADS * FR_OPEN_EVAL_MAX_BLOCKS               # the evaluation's largest grid: one stride of a thread
G = FR_OPEN_EVAL_GROUP
SIZES = [1, 2, 255, 256, 257, TMAX - 1, TMAX, TMAX + 1, 2 * TMAX + 1]
PERIOD = 4099                                                       # the shared data repeats 4099 random elements
LEN = 2 * TMAX + 1 + 4 * PERIOD                                     # room for slices that start at different offsets


class Bufs:
    """count buffers of n Fr side by side in one device allocation, a sentinel element before and after each"""

    def __init__(self, ctx, count, n):
        self.ctx, self.count, self.n = ctx, count, n
        self.host = np.full((count, n + 2, 4), SENT, dtype=np.uint64)
        self.dev = ctx.to_device(self.host)

    def ptr(self, i=0):
        return self.dev + 32 * ((self.n + 2) * i + 1)

    def fill(self, tables):
        """tables: count (n, 4) Montgomery arrays (None: sentinels)"""
        self.host[:] = SENT
        for i, t in enumerate(tables):
            if t is not None:
                self.host[i, 1:-1] = t
        self.ctx.h2d(self.dev, self.host)

    def read(self):
        out = np.zeros_like(self.host)
        self.ctx.d2h(out, self.dev)
        return out

    def expected(self, tables):
        exp = np.full_like(self.host, SENT)
        for i, t in enumerate(tables):
            if t is not None:
                exp[i, 1:-1] = t
        return exp

    def free(self):
        self.ctx.dev_free(self.dev)


def _mont(v, c):
    return codec.fr_to_mont(v, c)


def _r_words(c):
    return codec.ints_to_limbs([c.r], 4)[0]


class Shared:
    """One vector of LEN Fr on the device, shared by the evaluation and combination tests of a curve and never modified: a
    polynomial or a term is a slice (offset, length) of it.  pre[z][i] = sum_{k < i} x[k] z^k, so a slice evaluates to
    (pre[o + n] - pre[o]) / z^o."""

    def __init__(self, ctx, curve):
        self.ctx, self.c = ctx, get_curve(curve)
        r = self.c.r
        base = rand_fr(r, PERIOD, 77 + self.c.cid)
        base[0], base[3], base[255], base[256], base[1000] = r - 1, 0, 0, r - 1, 0
        idx = np.arange(LEN) % PERIOD
        self.x = [base[i] for i in idx.tolist()]
        self.words = _mont(base, self.c)[idx]
        self.dev = ctx.to_device(self.words)
        self.zs = {"zero": 0, "one": 1, "minus_one": r - 1, "random": rand_fr(r, 1, 5)[0]}
        self.pre = {}
        for name, z in self.zs.items():
            if z == 0:
                continue
            pre, acc, zp = [0] * (LEN + 1), 0, 1
            for i, v in enumerate(self.x):
                acc = (acc + v * zp) % r
                zp = zp * z % r
                pre[i + 1] = acc
            self.pre[name] = pre

    def ptr(self, off):
        return self.dev + 32 * off

    def eval(self, zname, off, n):
        r, z = self.c.r, self.zs[zname]
        if n == 0:
            return 0
        if z == 0:
            return self.x[off]
        return (self.pre[zname][off + n] - self.pre[zname][off]) * pow(z, -off, r) % r

    def unchanged(self):
        got = np.zeros_like(self.words)
        self.ctx.d2h(got, self.dev)
        return np.array_equal(got, self.words)


@pytest.fixture(scope="module")
def shared(ctx):
    out = {curve: Shared(ctx, curve) for curve in CURVES}
    yield out
    for s in out.values():
        ctx.dev_free(s.dev)


def _eval_many(ctx, c, ptrs, ns, z_words, count=None):
    """(status, the host output buffer with one sentinel row before and after the count rows)"""
    count = len(ns) if count is None else count
    m = max(len(ns), 1)
    pa = (ctypes.c_void_p * m)(*[p or None for p in ptrs])
    na = (ctypes.c_size_t * m)(*ns)
    out = np.full((max(count, 1) + 2, 4), SENT, dtype=np.uint64)
    z = np.ascontiguousarray(z_words, dtype=np.uint64)
    st = ctx.lib.zkp_fr_poly_eval_many_dev(ctx.h, c.cid, count, pa, na, z.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.c_void_p(out.ctypes.data + 32))
    return st, out


def _check_eval(ctx, sh, slices, znames=("zero", "one", "minus_one", "random")):
    """slices: (offset, length) per polynomial"""
    c = sh.c
    ptrs, ns = [sh.ptr(o) if n else 0 for o, n in slices], [n for _, n in slices]
    for zname in znames:
        st, out = _eval_many(ctx, c, ptrs, ns, codec.fr_mont(sh.zs[zname], c))
        assert st == 0, zname
        exp = np.full_like(out, SENT)
        exp[1:-1] = _mont([sh.eval(zname, o, n) for o, n in slices], c)
        assert np.array_equal(out, exp), (zname, slices)


# ------------------------------------------------------------------------------------------- evaluation at a shared point
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_eval_many_lengths(ctx, shared, curve, n):
    """one polynomial, and the same length beside shorter ones in a second register group"""
    sh = shared[curve]
    _check_eval(ctx, sh, [(0, n)])
    _check_eval(ctx, sh, [(7, min(n, 300)), (PERIOD + 1, n), (3, 1), (11, max(n - 1, 1)), (2, n)], znames=("random", "minus_one"))
    assert sh.unchanged()


@pytest.mark.parametrize("count", [1, G, G + 1, FR_OPEN_MAX_POLYS])
@pytest.mark.parametrize("curve", CURVES)
def test_eval_many_counts(ctx, shared, curve, count):
    sh = shared[curve]
    _check_eval(ctx, sh, [(13 * k, 700 + 37 * k) for k in range(count)])
    assert sh.unchanged()


@pytest.mark.parametrize("curve", CURVES)
def test_eval_many_mixed_lengths_and_repeated_pointers(ctx, shared, curve):
    """lengths 0 (NULL pointer), 1, below one block, above TMAX with the longest not first; one slice twice; a prefix of another"""
    sh = shared[curve]
    slices = [(5, 200), (0, 0), (9, 1), (PERIOD, 2 * TMAX + 1), (5, 200), (PERIOD, TMAX + 3), (0, 0), (40, 255), (1, TMAX)]
    _check_eval(ctx, sh, slices)
    _check_eval(ctx, sh, [(0, 0)] * 3, znames=("random",))           # every polynomial zero: one workgroup, all results 0
    assert sh.unchanged()


@pytest.mark.parametrize("curve", CURVES)
def test_eval_many_rules(ctx, shared, curve):
    sh = shared[curve]
    c = sh.c
    one = codec.fr_mont(1, c)

    def rejected(ptrs, ns, z, count=None):
        st, out = _eval_many(ctx, c, ptrs, ns, z, count)
        return st == BAD_ARG and (out == SENT).all()

    assert rejected([sh.ptr(0)], [8], one, count=0)
    many = FR_OPEN_MAX_POLYS + 1
    assert rejected([sh.ptr(0)] * many, [8] * many, one)
    assert rejected([sh.ptr(0), sh.ptr(4) + 8], [8, 8], one)          # a pointer off by 8 bytes
    assert rejected([sh.ptr(0), 0], [8, 8], one)                      # NULL with a length
    assert rejected([sh.ptr(0)], [(1 << 30) + 1], one)
    assert rejected([sh.ptr(0)], [8], _r_words(c))                    # z == r
    st, out = _eval_many(ctx, c, [sh.ptr(0), sh.ptr(4) + 8], [8, 0], one)      # a length of 0: the pointer is not looked at
    assert st == 0 and np.array_equal(out[1:-1], _mont([sh.eval("one", 0, 8), 0], c))
    assert sh.unchanged()


# ------------------------------------------------------------------------------------------- linear combination
def _lincomb_ref(sh, slices, scalars, n_out):
    r = sh.c.r
    out = [0] * n_out
    for (o, n), s in zip(slices, scalars):
        if s % r and n:
            seg = sh.x[o:o + n]
            out[:n] = [(a + s * b) % r for a, b in zip(out, seg)]
    return out


def _check_lincomb(ctx, sh, slices, scalars, n_out):
    c = sh.c
    out = Bufs(ctx, 1, n_out)
    try:
        out.fill([None])
        ctx.fr_lincomb_dev(c, [sh.ptr(o) if n else 0 for o, n in slices], [n for _, n in slices], _mont(scalars, c), out.ptr(), n_out)
        assert np.array_equal(out.read(), out.expected([_mont(_lincomb_ref(sh, slices, scalars, n_out), c)]))
    finally:
        out.free()


@pytest.mark.parametrize("n_out", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_lincomb_sizes(ctx, shared, curve, n_out):
    """a full-length term, a shorter one, one of length 0 (NULL) and one whose scalar is 0"""
    sh = shared[curve]
    s = rand_fr(sh.c.r, 2, n_out)
    _check_lincomb(ctx, sh, [(3, n_out), (PERIOD + 2, max(n_out // 2, 1)), (0, 0), (9, n_out)], [s[0], sh.c.r - 1, s[1], 0], n_out)
    assert sh.unchanged()


@pytest.mark.parametrize("count", [1, 2, 8, 20, FR_OPEN_MAX_POLYS])
@pytest.mark.parametrize("curve", CURVES)
def test_lincomb_counts_and_scalars(ctx, shared, curve, count):
    """mixed lengths (each term its own), scalars 0, 1, r - 1 among random ones, the output longer than every term"""
    sh = shared[curve]
    r = sh.c.r
    n_out = 777
    slices = [(17 * k, n_out - 19 * k if k % 3 else 300 + k) for k in range(count)]
    scalars = rand_fr(r, count, 3 + count)
    for k, v in zip(range(1, count, 3), (0, 1, r - 1) * 4):
        scalars[k] = v
    _check_lincomb(ctx, sh, slices, scalars, n_out)
    _check_lincomb(ctx, sh, slices, [1] * count, n_out)
    _check_lincomb(ctx, sh, slices, [0] * count, n_out)              # every term dropped: the output is zero-filled
    _check_lincomb(ctx, sh, [(0, 0)] * count, scalars, n_out)
    assert sh.unchanged()


@pytest.mark.parametrize("which", [0, 2, 4])
@pytest.mark.parametrize("curve", CURVES)
def test_lincomb_output_may_be_one_input(ctx, shared, curve, which):
    """out is the first, a middle or the last input itself; the other inputs are untouched"""
    sh = shared[curve]
    c, n = sh.c, 600
    lens = [n, 257, n, 1, n]
    lens[which] = n
    cols = [sh.x[100 * k:100 * k + n] for k in range(5)]
    scalars = rand_fr(c.r, 5, 40 + which)
    buf = Bufs(ctx, 5, n)
    try:
        tables = [_mont(v, c) for v in cols]
        buf.fill(tables)
        ctx.fr_lincomb_dev(c, [buf.ptr(k) for k in range(5)], lens, _mont(scalars, c), buf.ptr(which), n)
        exp = [0] * n
        for k in range(5):
            for i in range(lens[k]):
                exp[i] = (exp[i] + scalars[k] * cols[k][i]) % c.r
        tables[which] = _mont(exp, c)
        assert np.array_equal(buf.read(), buf.expected(tables))
    finally:
        buf.free()


@pytest.mark.parametrize("curve", CURVES)
def test_lincomb_rules(ctx, shared, curve):
    sh = shared[curve]
    c = sh.c
    buf = Bufs(ctx, 3, 64)
    try:
        buf.fill([_mont(rand_fr(c.r, 64, k), c) for k in range(3)])
        before = buf.read()
        p = [buf.ptr(0), buf.ptr(1)]
        one2 = _mont([1, 1], c)
        run = ctx.fr_lincomb_dev

        def status(*args):
            with pytest.raises(_lib.ZkpError) as e:
                run(c, *args)
            return e.value.status

        many = FR_OPEN_MAX_POLYS + 1
        assert status([], [], None, buf.ptr(2), 64) == BAD_ARG                                    # count 0
        assert status([p[0]] * many, [8] * many, _mont([1] * many, c), buf.ptr(2), 64) == BAD_ARG
        assert status([p[0], p[1] + 8], [8, 8], one2, buf.ptr(2), 64) == BAD_ARG                   # a pointer off by 8 bytes
        assert status(p, [8, 8], one2, buf.ptr(2) + 8, 16) == BAD_ARG
        assert status(p, [8, 65], one2, buf.ptr(2), 64) == BAD_ARG                                 # ns[k] > n_out
        assert status(p, [8, 8], one2, buf.ptr(2), 0) == BAD_ARG
        assert status(p, [64, 64], one2, p[1] + 32, 64) == BAD_ARG                                 # overlap at one element
        assert status(p, [64, 64], one2, p[1] - 32, 64) == BAD_ARG
        assert status(p, [64, 2], one2, p[1] + 32, 8) == BAD_ARG                                   # inside the span that is read
        assert status(p, [8, 8], np.stack([codec.fr_mont(1, c), _r_words(c)]), buf.ptr(2), 64) == BAD_ARG   # a scalar == r
        assert np.array_equal(buf.read(), before)                                                  # nothing ran
        run(c, p, [8, 2], one2, p[1] + 64, 8)                           # behind the two elements that are read: disjoint, fine
        after = buf.read()
        exp = before.copy()
        exp[1, 3:11] = _mont([(a + b) % c.r for a, b in zip(codec.fr_from_mont(before[0, 1:9], c),
                                                           codec.fr_from_mont(before[1, 1:3], c) + [0] * 6)], c)
        assert np.array_equal(after, exp)
    finally:
        buf.free()


# ------------------------------------------------------------------------------------------- driver: rounds 4 and 5
def _build(kind):
    return mini_circuit if kind == "mini" else (lambda cs: random_circuit(cs, kind, 60 + kind))


def _challenges(kind, r):
    return (MINI_CHALLENGES["beta"], MINI_CHALLENGES["gamma"], MINI_CHALLENGES["alpha"]) if kind == "mini" else challenges(r, kind)


def _reference(curve, kind, zeta, weights):
    rcs = _build(kind)(ref.RefComposer(curve))
    rix = ref.RefIndex(rcs, KS)
    ch = _challenges(kind, rcs.r)
    polys = ref.prove_rounds(rix, rcs.synthesize(), rcs.public_inputs(), *ch)
    assert polys["closes"]
    return rix, rcs, oref.run(rix, polys, rcs.public_inputs(), *ch, zeta, weights)


# 1500 gates: n = 2048, two blocks of the running product
@pytest.mark.parametrize("kind", ["mini", 37, 300, 1500])
@pytest.mark.parametrize("curve", CURVES)
def test_driver_rounds_4_and_5(ctx, curve, kind):
    c = get_curve(curve)
    golden = kind == "mini" and curve == "bls12_381"
    zeta = oref.MINI_ZETA % c.r if golden else rand_fr(c.r, 1, 31)[0]
    weights = oref.epsilon_weights(oref.MINI_EPSILON, c.r) if golden else dict(zip(oref.AT_ZETA, rand_fr(c.r, 10, 32)))
    rix, rcs, exp = _reference(curve, kind, zeta, weights)
    assert rix.n == {"mini": 8, 37: 64, 300: 512, 1500: 2048}[kind]
    ch = _challenges(kind, c.r)
    cs = _build(kind)(plonk.Composer(curve))
    ix = plonk.Index(ctx, curve, cs.compose(KS), KS, keep_coeffs=True)
    ps, out = None, Bufs(ctx, 1, ix.n)
    try:
        ps = plonk.prover_init(ix, cs.public_inputs())
        plonk.prover_first_round(ps, cs.synthesize(), to_host=False)
        plonk.prover_second_round(ps, ch[0], ch[1], to_host=False)
        plonk.prover_third_round(ps, ch[2], to_host=False)
        evals = plonk.prover_fourth_round(ps, zeta)
        assert list(evals) == list(oref.LABELS) == list(plonk.EVAL_LABELS)
        assert evals == exp["evals"]
        assert ps.base_evals == exp["base"] and len(ps.base_evals) == 21
        assert ps.terms == exp["terms"]
        assert plonk.linearisation_terms(curve, ix.n, KS, ps.base_evals, *ch, zeta) == exp["terms"]
        assert plonk.verifier_equality_check(curve, ix.n, evals, cs.public_inputs(), *ch, zeta)
        bad = dict(evals, r=(evals["r"] + 1) % c.r)
        assert not plonk.verifier_equality_check(curve, ix.n, bad, cs.public_inputs(), *ch, zeta)
        out.fill([None])
        plonk.linearisation_poly(ps, ps.terms, out.ptr())
        assert np.array_equal(out.read(), out.expected([_mont(exp["r_poly"], c)]))
        w_zeta, w_shifted = plonk.prover_openings(ps, zeta, weights=weights)
        assert w_zeta == exp["w_zeta"] and w_shifted == exp["w_shifted"]
        if golden:
            g = oref.load_golden()
            assert {k: str(v) for k, v in evals.items()} == g["evaluations"]
            assert [[str(s), label] for s, label in ps.terms] == g["r_terms"]
            assert [str(v) for v in w_zeta] == g["w_zeta"] and [str(v) for v in w_shifted] == g["w_shifted_zeta"]
            assert plonk.prover_openings(ps, zeta, epsilon=oref.MINI_EPSILON) == (w_zeta, w_shifted)
        for name in oref.PROVER:                                     # the inputs of rounds 4 and 5 are untouched
            assert ps.read(name) == exp["table"][name], name
        sel = np.zeros((ix.n, 4), dtype=np.uint64)
        for name in plonk.SELECTORS:
            ctx.d2h(sel, ix.coeffs[name])
            assert np.array_equal(sel, _mont(exp["table"][name], c)), name
    finally:
        out.free()
        if ps:
            ps.close()
        ix.close()


@pytest.mark.parametrize("curve", CURVES)
def test_round_4_needs_the_selector_coefficients(ctx, curve):
    c = get_curve(curve)
    ch = _challenges("mini", c.r)
    cs = mini_circuit(plonk.Composer(curve))
    ix = plonk.Index(ctx, curve, cs.compose(KS), KS)
    ps = None
    try:
        assert ix.coeffs == {} and len(ix.bufs) == 16
        ps = plonk.prover_init(ix, cs.public_inputs())
        plonk.prover_first_round(ps, cs.synthesize(), to_host=False)
        plonk.prover_second_round(ps, ch[0], ch[1], to_host=False)
        plonk.prover_third_round(ps, ch[2], to_host=False)
        with pytest.raises(ValueError, match="keep_coeffs"):
            plonk.prover_fourth_round(ps, 5)
    finally:
        if ps:
            ps.close()
        ix.close()


@pytest.mark.parametrize("curve", CURVES)
def test_prove_commits_and_opens(ctx, curve):
    """prove() with a key of known beta: every commitment is [p(beta)] G and both witness commitments are [W(beta)] G, with p and
    W from the reference's coefficients (no pairing needed)"""
    c = get_curve(curve)
    kind, tau = 37, 0x5EED0FC0FFEE12345
    fixed = dict(zip((1, 2, 3, 4), (challenges(c.r, kind)[:2], challenges(c.r, kind)[2], rand_fr(c.r, 1, 33)[0], rand_fr(c.r, 1, 34)[0])))
    seen = []

    def challenge(stage, payload):
        seen.append((stage, list(payload)))
        return fixed[stage]

    rix, rcs, exp = _reference(curve, kind, fixed[3], oref.epsilon_weights(fixed[4], c.r))
    cs = _build(kind)(plonk.Composer(curve))
    ix = plonk.Index(ctx, curve, cs.compose(KS), KS, keep_coeffs=True)
    ck = kzg10.setup(ctx, curve, ix.n - 1, tau)
    try:
        proof = plonk.prove(ctx, ck, ix, cs.synthesize(), cs.public_inputs(), challenge)
    finally:
        ck.powers_of_g.free()
        ck.powers_of_gamma_g.free()
        ix.close()
    assert [s for s, _ in seen] == [1, 2, 3, 4]
    assert seen[0][1] == list(oref.PROVER[:4]) and seen[1][1] == list(oref.PROVER[:5]) and seen[2][1] == list(oref.PROVER)
    assert seen[3][1] == list(oref.LABELS)
    assert proof["evaluations"] == exp["evals"] and list(proof["evaluations"]) == list(oref.LABELS)
    g1 = Group(OC[curve], 1)
    at_tau = lambda p: g1.mul(g1.gen, ref.horner(p, tau, c.r))       # noqa: E731
    assert list(proof["commitments"]) == list(oref.PROVER)
    for name in oref.PROVER:
        assert proof["commitments"][name] == at_tau(exp["table"][name]), name
    assert proof["witnesses"] == (at_tau(exp["w_zeta"]), at_tau(exp["w_shifted"]))
