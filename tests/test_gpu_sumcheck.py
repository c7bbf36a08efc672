"""zkp_fr_sumcheck_round_dev / zkp_fr_eq_evals_dev / ckb_zkp_amd.sumcheck on the device, bit-exact against tests/sumcheck_ref.py
(Python integers that follow spartan/src/polynomial.rs and prover.rs) and, at full size, against oracle/cpu's fr_dot.
test_round_more_workgroups_than_sum_threads (2 SC_THREADS workgroups under fr_sum_partials, one round checked on its own, also
with ZKP_TEST_FULL=0) takes about 0.1 s a case on an MI355X."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from ckb_zkp_amd import api, codec, sumcheck
from ckb_zkp_amd.params import get_curve
from oracle import cpu_oracle
from tests import sumcheck_ref as ref
from tests.util import TEST_FULL, csrc_constant, periodic_bind, periodic_round_sums

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
KINDS = [api.SC_EQ_AB_MINUS_C, api.SC_PROD2, api.SC_PROD3]
SENT = 0xABABABABABABABAB
SC_THREADS = csrc_constant("sumcheck.hip", "SC_THREADS")         # threads of sc_round_kernel and of its fr_sum_partials
PERIOD = 1021                                                      # long tables repeat a block of this (prime) length
STEP = 37                                                          # table i of a case is pool[STEP i : STEP i + len]


def _pool(c, n, seed):
    """n field elements as (integers, (n, 4) Montgomery words); 0 and r - 1 among them"""
    rng = np.random.default_rng(seed)
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)      # < 2^(bits - 1) < r
    ints = codec.limbs_to_ints(k)
    for i in range(0, n, 29):
        ints[i] = 0
    for i in range(5, n, 31):
        ints[i] = c.r - 1
    return ints, codec.fr_to_mont(ints, c)


class Tables:
    """ntab tables of n elements each, side by side in one device buffer, cut from one pool at different offsets"""

    def __init__(self, ctx, c, ntab, n, seed):
        self.ctx, self.c, self.ntab, self.n = ctx, c, ntab, n
        pool, words = _pool(c, n + STEP * ntab, seed)
        self.pool = pool
        self.ints = [pool[STEP * i:STEP * i + n] for i in range(ntab)]
        self.words = np.ascontiguousarray(np.stack([words[STEP * i:STEP * i + n] for i in range(ntab)]))
        self.dev = ctx.dev_alloc(self.words.nbytes)
        self.upload()

    def upload(self):
        self.ctx.h2d(self.dev, self.words)

    def ptr(self, i):
        return self.dev + 32 * self.n * i

    def read(self):
        out = np.zeros_like(self.words)
        self.ctx.d2h(out, self.dev)
        return out

    def bound(self, x):
        """(integers, Montgomery words) of combine_with_r(table, x) for every table: the tables are windows of the pool, so their
        bound halves are windows of pool[p] bound with pool[p + n / 2]"""
        h, r = self.n // 2, self.c.r
        assert ref.combine_with_r(self.ints[-1], x, r)[:64] == [(lo + x * (hi - lo)) % r for lo, hi in
                                                                 zip(self.ints[-1][:h][:64], self.ints[-1][h:])]
        bp = [(lo + x * (hi - lo)) % r for lo, hi in zip(self.pool, self.pool[h:])]
        bw = codec.fr_to_mont(bp, self.c)
        span = range(self.ntab)
        return [bp[STEP * i:STEP * i + h] for i in span], np.stack([bw[STEP * i:STEP * i + h] for i in span])

    def free(self):
        self.ctx.dev_free(self.dev)


def _ints(c, ev):
    return [tuple(codec.fr_from_mont(term, c)) for term in ev]


def _m(c, x):
    return codec.fr_to_mont([x], c)[0]


# ------------------------------------------------------------------------------------------- eq table
@pytest.mark.parametrize("curve,k", [(cv, k) for cv in CURVES for k in (0, 1, 2, 7, 10, 16)] + [("bn254", 20)])
def test_eq_table(ctx, curve, k):
    c = get_curve(curve)
    rs = _pool(c, max(k, 1), 100 + k)[0][:k]
    for i, v in zip(range(0, k, 2), (c.r - 1, 0, 1) * 4):           # every k >= 1 sees r - 1, k >= 3 also 0, k >= 5 also 1
        rs[i] = v
    got = ctx.fr_eq_evals(c, codec.fr_to_mont(rs, c).reshape(-1, 4))
    assert got.shape == (1 << k, 4)
    assert np.array_equal(got, codec.fr_to_mont(ref.eval_eq(rs, c.r), c))


# ------------------------------------------------------------------------------------------- one round
@pytest.mark.parametrize("n", [2, 4, 8, 128, 512, 1024, 2048, 4096, 1 << 16])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("curve", CURVES)
def test_round(ctx, curve, kind, n):
    c = get_curve(curve)
    r = c.r
    ar = ref.ARITY[kind]
    for count in (1, 3, 17):
        t = Tables(ctx, c, count * ar, n, seed=1000 * kind + count)
        try:
            ptrs = [t.ptr(i) for i in range(count * ar)]
            x = t.ints[0][1] if n > 2 else 12345
            b_ints, b_words = t.bound(x)
            h = n // 2
            # evaluation only: the tables stay as they are
            ev = ctx.fr_sumcheck_round_dev(c, kind, ptrs, n)
            assert _ints(c, ev) == [ref.round_evals(kind, t.ints[k * ar:(k + 1) * ar], r) for k in range(count)], (count, "eval")
            assert np.array_equal(t.read(), t.words)
            # bind only
            assert ctx.fr_sumcheck_round_dev(c, kind, ptrs, n, bind=_m(c, x), want_evals=False) is None
            got = t.read()
            assert np.array_equal(got[:, :h], b_words), (count, "bind")
            assert np.array_equal(got[:, h:], t.words[:, h:]), (count, "bind: high half")
            if n < 4:
                continue
            # bind + evaluate
            t.upload()
            ev = ctx.fr_sumcheck_round_dev(c, kind, ptrs, n, bind=_m(c, x))
            assert _ints(c, ev) == [ref.round_evals(kind, b_ints[k * ar:(k + 1) * ar], r) for k in range(count)], (count, "fused")
            got = t.read()
            assert np.array_equal(got[:, :h], b_words), (count, "fused: low half")
            assert np.array_equal(got[:, h:], t.words[:, h:]), (count, "fused: high half")
        finally:
            t.free()


@pytest.mark.parametrize("curve", CURVES)
def test_shared_tables(ctx, curve):
    c = get_curve(curve)
    r = c.r
    n = 1024
    t = Tables(ctx, c, 12, n, seed=77)
    try:
        # PROD3: terms 0, 2, 4 share table 6 as c (the `par` shape); term 1 is d d e; term 3 shares e with term 1; term 5 is d d d
        idx = [(0, 1, 6), (7, 7, 8), (2, 3, 6), (9, 10, 8), (4, 5, 6), (11, 11, 11)]
        ptrs = [t.ptr(i) for term in idx for i in term]
        x = t.ints[3][9]
        b_ints, b_words = t.bound(x)
        ev = ctx.fr_sumcheck_round_dev(c, api.SC_PROD3, ptrs, n, bind=_m(c, x))
        assert _ints(c, ev) == [ref.round_evals(ref.PROD3, [b_ints[i] for i in term], r) for term in idx]
        first = t.read()
        assert np.array_equal(first[:, :n // 2], b_words)             # bound once, not once per use
        assert np.array_equal(first[:, n // 2:], t.words[:, n // 2:])
        t.upload()
        again = ctx.fr_sumcheck_round_dev(c, api.SC_PROD3, ptrs, n, bind=_m(c, x))
        assert again.tobytes() == ev.tobytes() and t.read().tobytes() == first.tobytes()
        # a a (PROD2) beside a b with the same a; eq a a c (phase-one shape with b = a); evaluation only and bind only as well
        t.upload()
        ev = ctx.fr_sumcheck_round_dev(c, api.SC_PROD2, [t.ptr(0), t.ptr(0), t.ptr(0), t.ptr(1)], n, bind=_m(c, x))
        assert _ints(c, ev) == [ref.round_evals(ref.PROD2, [b_ints[0], b_ints[0]], r), ref.round_evals(ref.PROD2, [b_ints[0], b_ints[1]], r)]
        got = t.read()
        assert np.array_equal(got[:2, :n // 2], b_words[:2]) and np.array_equal(got[2:], t.words[2:])
        t.upload()
        four = [t.ptr(2), t.ptr(3), t.ptr(3), t.ptr(4)]
        ev = ctx.fr_sumcheck_round_dev(c, api.SC_EQ_AB_MINUS_C, four, n)
        assert _ints(c, ev) == [ref.round_evals(ref.EQ_AB_MINUS_C, [t.ints[2], t.ints[3], t.ints[3], t.ints[4]], r)]
        ctx.fr_sumcheck_round_dev(c, api.SC_EQ_AB_MINUS_C, four, n, bind=_m(c, x), want_evals=False)
        got = t.read()
        assert np.array_equal(got[2:5, :n // 2], b_words[2:5]) and np.array_equal(got[2:5, n // 2:], t.words[2:5, n // 2:])
    finally:
        t.free()


@pytest.mark.parametrize("bind", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_round_more_workgroups_than_sum_threads(ctx, curve, bind):
    """2^18 elements without a bind, 2^19 with one: h = 2^17 columns in 2 SC_THREADS workgroups, the fewest at which a thread of
    fr_sum_partials adds a second partial of sc_round_kernel's layout (out NP + p) gridDim.x + blockIdx.x.  Two SC_EQ_AB_MINUS_C
    terms share their eq table, so they run in one group and the second term's partials lie behind the first's.  The tables repeat
    PERIOD values each: the sums are formed per residue (tests/util.periodic_round_sums over ref.round_evals), the bound halves
    repeat periodic_bind's block.  One sentinel element before the first and after the last table."""
    c = get_curve(curve)
    r, kind = c.r, api.SC_EQ_AB_MINUS_C
    n = 1 << (19 if bind else 18)
    h = n // (4 if bind else 2)
    assert SC_THREADS < h // SC_THREADS <= 2 * SC_THREADS and (h // 2) // SC_THREADS <= SC_THREADS
    terms = [(0, 1, 2, 3), (0, 4, 5, 6)]
    rng = random.Random(f"{curve} {bind}")
    bases = [[rng.randrange(r) for _ in range(PERIOD)] for _ in range(7)]
    for b in bases:
        b[3], b[5] = 0, r - 1
    x = rng.randrange(2, r)
    idx = np.arange(n) % PERIOD
    sent = np.full((1, 4), SENT, dtype=np.uint64)
    host = np.concatenate([sent] + [codec.fr_to_mont(b, c)[idx] for b in bases] + [sent])
    dev = ctx.to_device(host)
    try:
        ptrs = [dev + 32 * (1 + n * i) for term in terms for i in term]
        exp = host.copy()
        if bind:
            bases = [periodic_bind(b, n // 2, x, r) for b in bases]
            for i, b in enumerate(bases):
                exp[1 + n * i:1 + n * i + n // 2] = codec.fr_to_mont(b, c)[idx[:n // 2]]     # the upper half untouched
        ev = ctx.fr_sumcheck_round_dev(c, kind, ptrs, n, bind=_m(c, x) if bind else None)
        want = [periodic_round_sums(lambda t: ref.round_evals(kind, t, r), [bases[i] for i in term], h, r) for term in terms]
        assert _ints(c, ev) == want
        got = np.zeros_like(host)
        ctx.d2h(got, dev)
        assert np.array_equal(got, exp)
    finally:
        ctx.dev_free(dev)


# ------------------------------------------------------------------------------------------- argument rules
@pytest.mark.parametrize("curve", CURVES)
def test_errors_leave_everything_untouched(ctx, curve):
    c = get_curve(curve)
    n = 64
    V = ctypes.c_void_p
    words = np.full((6, n, 4), SENT, dtype=np.uint64)
    dev = ctx.to_device(words)
    out = np.full((257 * 3, 4), SENT, dtype=np.uint64)
    good = _m(c, 5)
    big = np.frombuffer(c.r.to_bytes(32, "little"), dtype=np.uint64).copy()      # r: not reduced
    tab = [dev + 32 * n * i for i in range(6)]
    fn = ctx.lib.zkp_fr_sumcheck_round_dev
    eq = ctx.lib.zkp_fr_eq_evals_dev
    kp = lambda a: None if a is None else V(a.ctypes.data)        # noqa: E731
    base = dict(cu=c.cid, kind=0, t=tab[:4], n=n, x=good, o=out)

    def call(**kw):
        a = dict(base, **kw)
        arr = None if a["t"] is None else (V * max(len(a["t"]), 1))(*[p or None for p in a["t"]])
        count = a.get("count", 0 if a["t"] is None else len(a["t"]) // ref.ARITY.get(a["kind"], 4))
        return fn(ctx.h, a["cu"], a["kind"], count, arr, a["n"], kp(a["x"]), kp(a["o"]))
    try:
        bad = [dict(t=None, count=1), dict(t=[tab[0], 0, tab[2], tab[3]]),                    # NULL array, NULL table
               dict(t=[tab[0], tab[1] + 8, tab[2], tab[3]]),                                    # misaligned
               dict(n=0), dict(n=6), dict(n=48), dict(n=1 << 29),                               # not a power of two, too long
               dict(n=1, o=None), dict(n=1, x=None), dict(n=2),                                 # below 2 to bind / to evaluate
               dict(x=None, o=None),                                                            # nothing to do
               dict(kind=3, t=tab[:4]), dict(kind=-1, t=tab[:4]),                               # unknown kind
               dict(x=big),                                                                     # challenge >= r
               dict(kind=1, t=[tab[0], tab[1]] * 257),                                          # count > 256
               dict(t=[tab[0], tab[0] + 32, tab[2], tab[3]]), dict(t=[tab[1], tab[2], tab[3], tab[2] - 32 * (n - 1)]),   # overlap
               dict(kind=1, t=[tab[0], tab[1], tab[1] + 16, tab[5]])]
        for kw in bad:
            assert call(**kw) == -1, kw
        assert call(cu=7) == -2
        assert call(t=None, count=0) == 0
        # eq table
        rs = np.stack([good, good, good])
        e = lambda cu, r_, k, o: eq(ctx.h, cu, kp(r_), k, V(o))   # noqa: E731
        assert e(c.cid, rs, 29, dev) == -1
        assert e(c.cid, np.stack([good, big, good]), 3, dev) == -1
        assert e(c.cid, rs, 3, 0) == -1
        assert e(c.cid, rs, 3, dev + 8) == -1
        assert e(c.cid, None, 3, dev) == -1
        assert e(7, rs, 3, dev) == -2
        chk = np.zeros_like(words)
        ctx.d2h(chk, dev)
        assert (chk == SENT).all() and (out == SENT).all()
        # good calls on real data
        t = Tables(ctx, c, 4, n, seed=5)
        try:
            base["t"] = [t.ptr(i) for i in range(4)]
            assert call() == 0
            assert [tuple(codec.fr_from_mont(out[:3], c))] == [ref.round_evals(0, t.bound(5)[0], c.r)]
            assert (out[3:] == SENT).all()
        finally:
            t.free()
        assert e(c.cid, rs, 3, dev) == 0
        ctx.d2h(chk, dev)
        assert np.array_equal(chk[0, :8], codec.fr_to_mont(ref.eval_eq([5, 5, 5], c.r), c)) and (chk[0, 8:] == SENT).all()
    finally:
        ctx.dev_free(dev)


# ------------------------------------------------------------------------------------------- whole provers
def _challenge(c, tag=b""):
    def ch(coeffs):
        h = hashlib.sha256(tag + b"".join(int(v).to_bytes(32, "little") for v in coeffs)).digest()
        return int.from_bytes(h, "little") % c.r
    return ch


@pytest.mark.parametrize("curve", CURVES)
def test_phase_one_and_two(ctx, curve):
    c = get_curve(curve)
    r = c.r
    n = 256
    t = Tables(ctx, c, 4, n, seed=41)
    try:
        eq, a, b, cc = t.ints
        claim = sum(e * (x * y - z) for e, x, y, z in zip(eq, a, b, cc)) % r
        got = sumcheck.prove_phase_one(ctx, c, t.ptr(0), t.ptr(1), t.ptr(2), t.ptr(3), n, claim, _challenge(c))
        assert got == ref.phase_one(eq, a, b, cc, claim, _challenge(c), r)
        polys, rx, (va, vb, vc, veq) = got
        assert ref.evaluate(polys[-1], rx[-1], r) == veq * (va * vb - vc) % r
        t.upload()
        claim = sum(x * y for x, y in zip(a, b)) % r
        got = sumcheck.prove_phase_two(ctx, c, t.ptr(1), t.ptr(2), n, claim, _challenge(c, b"2"))
        assert got == ref.phase_two(a, b, claim, _challenge(c, b"2"), r)
        assert ref.evaluate(got[0][-1], got[1][-1], r) == got[2][0] * got[2][1] % r
    finally:
        t.free()


@pytest.mark.parametrize("curve", CURVES)
def test_cubic_batched(ctx, curve):
    c = get_curve(curve)
    r = c.r
    n = 128
    t = Tables(ctx, c, 13, n, seed=43)                             # 3 par (a, b) + c_par + 2 seq (a, b, c)
    try:
        T, P = t.ints, t.ptr
        coeffs = _pool(c, 5, 44)[0]
        par_i, seq_i = [(0, 1), (2, 3), (4, 5)], [(7, 8, 9), (10, 11, 12)]
        claim = (sum(w * sum(x * y * z for x, y, z in zip(T[i], T[j], T[6])) for w, (i, j) in zip(coeffs, par_i))
                 + sum(w * sum(x * y * z for x, y, z in zip(T[i], T[j], T[k])) for w, (i, j, k) in zip(coeffs[3:], seq_i))) % r
        got = sumcheck.prove_cubic_batched(ctx, c, [(P(i), P(j)) for i, j in par_i], P(6), [tuple(P(i) for i in s) for s in seq_i],
                                           coeffs, n, claim, _challenge(c))
        exp = ref.cubic_batched([T[i] for i, _ in par_i], [T[j] for _, j in par_i], T[6], [T[s[0]] for s in seq_i],
                                [T[s[1]] for s in seq_i], [T[s[2]] for s in seq_i], coeffs, claim, _challenge(c), r)
        assert got == exp
    finally:
        t.free()


def _r1cs(c, rows, nz, seed, satisfied):
    """random sparse A, B and a C with Cz = Az o Bz (one entry per row), as rows of (value, column); z integers"""
    r = c.r
    rng = np.random.default_rng(seed)
    vals = iter(_pool(c, 8 * rows + nz, seed)[0])
    z = [next(vals) or 1 for _ in range(nz)]
    sparse = lambda: [[(next(vals), int(rng.integers(nz))) for _ in range(int(rng.integers(1, 4)))] for _ in range(rows)]   # noqa: E731
    ma, mb = sparse(), sparse()
    ma[3] = []                                                     # an empty row
    az, bz = ref.matrix_vec(ma, z, r), ref.matrix_vec(mb, z, r)
    mc = [[(x * y * pow(z[i + 1], -1, r) % r, i + 1)] for i, (x, y) in enumerate(zip(az, bz))]
    if not satisfied:
        mc[5] = [(mc[5][0][0] + 1, mc[5][0][1])]
    return ma, mb, mc, z


def _csr(c, m):
    row_ptr = np.cumsum([0] + [len(row) for row in m]).astype(np.uint32)
    col = np.array([cl for row in m for _, cl in row], dtype=np.uint32)
    return row_ptr, col, codec.fr_to_mont([v for row in m for v, _ in row], c)


@pytest.mark.parametrize("satisfied", [True, False])
@pytest.mark.parametrize("curve", CURVES)
def test_r1cs_sumcheck(ctx, curve, satisfied):
    c = get_curve(curve)
    r = c.r
    rows, nz = 64, 128
    ma, mb, mc, z = _r1cs(c, rows, nz, 51, satisfied)
    tau = _pool(c, 6, 52)[0]
    abc = lambda va, vb, vc, veq: tuple(_challenge(c, bytes([i]))([va, vb, vc, veq]) for i in range(3))   # noqa: E731
    got = sumcheck.r1cs_sumcheck(ctx, c, _csr(c, ma), _csr(c, mb), _csr(c, mc), codec.fr_to_mont(z, c), tau, _challenge(c, b"x"), abc,
                                 _challenge(c, b"y"))
    exp = ref.r1cs_backbone(ma, mb, mc, z, tau, _challenge(c, b"x"), abc, _challenge(c, b"y"), r)
    assert got == exp
    p1, rx, (va, vb, vc, veq), p2, ry, (vs, vz) = got
    # g(1) is derived from the claim, so a false claim only shows at the end: the last claim is not the product of the finals
    assert (ref.evaluate(p1[-1], rx[-1], r) == veq * (va * vb - vc) % r) == satisfied
    assert ref.evaluate(p2[-1], ry[-1], r) == vs * vz % r


def test_phase_one_full_size(ctx):
    """2^20 BN254 (ZKP_TEST_FULL=0: 2^16): a satisfied instance against the Python reference, and va = <a, eq(rx)> through
    oracle/cpu independently of it"""
    c = get_curve("bn254")
    r = c.r
    k = 20 if TEST_FULL else 16
    n = 1 << k
    pool, words = _pool(c, n + STEP, 61)
    a, b = pool[:n], pool[STEP:STEP + n]
    cc = [x * y % r for x, y in zip(a, b)]
    tau = _pool(c, k, 62)[0]
    a_words = np.ascontiguousarray(words[:n])
    bufs = [ctx.to_device(a_words), ctx.to_device(np.ascontiguousarray(words[STEP:STEP + n])), ctx.to_device(codec.fr_to_mont(cc, c)),
            ctx.dev_alloc(32 * n)]
    try:
        da, db, dc, de = bufs
        ctx.fr_eq_evals_dev(c, codec.fr_to_mont(tau, c), de)
        got = sumcheck.prove_phase_one(ctx, c, de, da, db, dc, n, 0, _challenge(c))
        polys, rx, (va, vb, vc, veq) = got
        assert va == cpu_oracle.fr_dot(c, a_words, codec.fr_to_mont(ref.eval_eq(rx, r), c))
        assert veq == ref.eval_eq_x_y(tau, rx, r)
        assert ref.evaluate(polys[-1], rx[-1], r) == veq * (va * vb - vc) % r
        assert got == ref.phase_one(ref.eval_eq(tau, r), a, b, cc, 0, _challenge(c), r)
    finally:
        for p in bufs:
            ctx.dev_free(p)
