"""zkp_fr_powers_dev / zkp_fr_bp_t_coeffs_dev / zkp_fr_bp_lr_eval_dev / zkp_fr_ipa_fold_ab_dev and ckb_zkp_amd.bulletproofs on the device,
bit-exact against tests/bulletproofs_ref.py (Python integers).  0 and r - 1 are among the operands.  Every writable buffer starts
as sentinels with one sentinel element before and after it, whole buffers are compared, and the inputs are read back unchanged.
Every input vector is followed by nonzero padding that the kernels must not read."""
import numpy as np
import pytest

from ckb_zkp_amd import _lib, bulletproofs, codec
from ckb_zkp_amd.bulletproofs import BP_MAX_GROUPS, BP_THREADS
from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.r1cs import R1csInstance
from tests import bulletproofs_ref as ref
from tests.bulletproofs_cases import (MINI_CURVE, Challenger, assert_same_proof, generators, load_golden, mini, mini_setup,
                                      proof_to_json, random_circuit, randomness)
from tests.gkr_cases import rand_fr
from tests.test_gpu_gkr import SENT, Bufs

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
T_MAX = BP_THREADS * BP_MAX_GROUPS          # threads of the largest pass: index T_MAX is the first second index of a thread
PERIOD = 1021                               # long vectors repeat a block of this (prime) length: cheap to encode, no power-of-two stride
PAD = 3                                     # nonzero elements after every input vector


def _bad_arg(fn):
    with pytest.raises(_lib.ZkpError) as e:
        fn()
    assert e.value.status == -1


def _values(c, n, seed):
    """n integers of period PERIOD with 0 and r - 1 among them, and their Montgomery words"""
    base = rand_fr(c.r, min(n, PERIOD), seed)
    if base:
        base[0] = 0
        base[-1] = c.r - 1
    if len(base) > 2:
        base[1] = c.r - 1
    idx = np.arange(n) % PERIOD
    words = codec.fr_to_mont(base, c)[idx] if n else np.zeros((0, 4), dtype=np.uint64)
    return [base[i] for i in idx], words


class Inputs:
    """the seven vectors of a zkp_bp_vectors side by side in one allocation: sentinel, the vector, PAD nonzero elements, sentinel"""

    def __init__(self, ctx, c, n, n_w, n_s, N, seed, null_empty=True):
        self.ctx, self.lens = ctx, [n, n, n, n_w, n_w, n_s, n_s]
        self.ints, parts, self.offs = [], [], []
        pad = codec.fr_to_mont([5, c.r - 1, 7], c)
        sent = np.full((1, 4), SENT, dtype=np.uint64)
        at = 0
        for i, ln in enumerate(self.lens):
            ints, words = _values(c, ln, seed + i)
            self.ints.append(ints)
            parts += [sent, words, pad, sent]
            self.offs.append(at + 1)
            at += ln + PAD + 2
        self.host = np.concatenate(parts)
        self.dev = ctx.to_device(self.host)
        ptrs = [self.dev + 32 * o if (ln or not null_empty) else 0 for o, ln in zip(self.offs, self.lens)]
        self.ptrs = ptrs
        self.vecs = ctx.bp_vectors(*ptrs, n, n_w, n_s, N)

    def unchanged(self):
        got = np.zeros_like(self.host)
        self.ctx.d2h(got, self.dev)
        return np.array_equal(got, self.host)

    def free(self):
        self.ctx.dev_free(self.dev)


# ------------------------------------------------------------------------------------------- powers
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, T_MAX + 1])
@pytest.mark.parametrize("curve", CURVES)
def test_powers(ctx, curve, n):
    """T_MAX + 1: the smallest n at which a thread (thread 0) owns two indices"""
    c = get_curve(curve)
    r = c.r
    out = Bufs(ctx, 1, max(n, 1))
    firsts = [r - 1, 1, rand_fr(r, 1, 9)[0], r - 2]
    try:
        for first, ratio in zip(firsts, [0, 1, r - 1, rand_fr(r, 1, n)[0]]):
            out.fill(c, [None])
            ctx.fr_powers_dev(c, codec.fr_mont(first, c), codec.fr_mont(ratio, c), out.ptr(0), n)
            exp, x = [], first
            for _ in range(n):
                exp.append(x)
                x = x * ratio % r
            want = np.full_like(out.host, SENT)
            if n:
                want[0, 1:1 + n] = codec.fr_to_mont(exp, c)
            assert np.array_equal(out.read(), want), (n, ratio)
    finally:
        out.free()


def test_powers_zero_ratio_and_argument_rules(ctx):
    c = get_curve("bn254")
    out = Bufs(ctx, 1, 4)
    one, rr = codec.fr_mont(1, c), codec.ints_to_limbs([c.r], 4)[0]
    try:
        out.fill(c, [None])
        ctx.fr_powers_dev(c, codec.fr_mont(6, c), codec.fr_mont(0, c), out.ptr(0), 4)
        assert np.array_equal(out.read(), out.expected(c, [[6, 0, 0, 0]]))
        out.fill(c, [None])
        _bad_arg(lambda: ctx.fr_powers_dev(c, rr, one, out.ptr(0), 4))
        _bad_arg(lambda: ctx.fr_powers_dev(c, one, rr, out.ptr(0), 4))
        _bad_arg(lambda: ctx.fr_powers_dev(c, one, one, out.ptr(0) + 8, 2))
        _bad_arg(lambda: ctx.fr_powers_dev(c, one, one, out.ptr(0), (1 << 28) + 1))
        assert np.array_equal(out.read(), out.expected(c, [None]))
    finally:
        out.free()


# ------------------------------------------------------------------------------------------- l(X), r(X)
SHAPES = [(1, 1, 1, 1), (1, 0, 1, 2), (3, 2, 3, 4), (10, 2, 10, 16), (2, 5, 5, 8), (64, 64, 64, 64), (200, 7, 200, 256), (257, 300, 300, 512)]


def _check_lr(ctx, curve, shape, seed):
    c = get_curve(curve)
    r = c.r
    n, n_w, n_s, N = shape
    inp = Inputs(ctx, c, n, n_w, n_s, N, seed)
    out = Bufs(ctx, 2, N)
    try:
        if n_w == 0:
            assert inp.vecs.w is None and inp.vecs.v is None        # NULL where the length is 0
        y, z, x = rand_fr(r, 3, seed + 100)
        if seed % 2:
            z = r - 1
        ym, zm, xm = (codec.fr_mont(v, c) for v in (y, z, x))
        lp, rp = ref.lr_from_vectors(*inp.ints, N, y, z, r)
        t_ref = ref.t_coeffs(lp, rp, r)
        t = [codec.fr_int(e, c) for e in ctx.fr_bp_t_coeffs_dev(c, inp.vecs, ym, zm)]
        assert t == [t_ref[d] for d in range(2, 11)]
        out.fill(c, [None, None])
        t_x = codec.fr_int(ctx.fr_bp_lr_eval_dev(c, inp.vecs, ym, zm, xm, out.ptr(0), out.ptr(1)), c)
        l_x, r_x = ref.eval_vec_poly(lp, x, r), ref.eval_vec_poly(rp, x, r)
        assert np.array_equal(out.read(), out.expected(c, [l_x, r_x]))
        assert t_x == ref.dot(l_x, r_x, r)
        assert t_x == sum(t[d - 2] * pow(x, d, r) for d in range(2, 11)) % r       # the first call's coefficients at x
        assert inp.unchanged()
    finally:
        out.free()
        inp.free()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_t_coeffs_and_lr_eval(ctx, curve, shape):
    _check_lr(ctx, curve, shape, sum(shape) + len(curve))


def test_t_coeffs_and_lr_eval_two_indices_per_thread(ctx):
    N = 2 * T_MAX
    _check_lr(ctx, "bn254", (N // 2 + 1, 5, T_MAX + 2, N), 17)


def test_lr_argument_rules(ctx):
    c = get_curve("bls12_381")
    r = c.r
    n, n_w, n_s, N = 3, 2, 3, 4
    inp = Inputs(ctx, c, n, n_w, n_s, N, 5)
    out = Bufs(ctx, 2, N)
    t_out = np.full((9, 4), SENT, dtype=np.uint64)
    tx_out = np.full(4, SENT, dtype=np.uint64)
    lib, V = ctx.lib, _lib.C.c_void_p
    good, zero, rr = codec.fr_mont(12345, c), codec.fr_mont(0, c), codec.ints_to_limbs([r], 4)[0]

    def t_call(vecs, y, z):
        return lib.zkp_fr_bp_t_coeffs_dev(ctx.h, c.cid, _lib.C.byref(vecs), V(y.ctypes.data), V(z.ctypes.data), V(t_out.ctypes.data))

    def lr_call(vecs, y, z, x, l_ptr, r_ptr):
        return lib.zkp_fr_bp_lr_eval_dev(ctx.h, c.cid, _lib.C.byref(vecs), V(y.ctypes.data), V(z.ctypes.data), V(x.ctypes.data),
                                         V(l_ptr), V(r_ptr), V(tx_out.ctypes.data))

    def vecs_with(**kw):
        v = ctx.bp_vectors(*inp.ptrs, n, n_w, n_s, N)
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    try:
        out.fill(c, [None, None])
        lo, ro = out.ptr(0), out.ptr(1)
        assert t_call(inp.vecs, good, good) == 0 and lr_call(inp.vecs, good, good, good, lo, ro) == 0     # the calls are sound
        out.fill(c, [None, None])
        t_out[:] = SENT
        tx_out[:] = SENT
        bad_vecs = [vecs_with(N=6), vecs_with(N=0), vecs_with(n=N + 1), vecs_with(n_w=N + 1), vecs_with(n_s=N + 1),
                    vecs_with(aR=inp.ptrs[1] + 8), vecs_with(sL=inp.ptrs[5] + 4), vecs_with(v=None), vecs_with(N=1 << 29)]
        for v in bad_vecs:
            assert t_call(v, good, good) == -1
            assert lr_call(v, good, good, good, lo, ro) == -1
        for y, z in ((zero, good), (rr, good), (good, rr)):
            assert t_call(inp.vecs, y, z) == -1
            assert lr_call(inp.vecs, y, z, good, lo, ro) == -1
        assert lr_call(inp.vecs, good, good, rr, lo, ro) == -1
        assert lr_call(inp.vecs, good, good, good, lo + 8, ro) == -1                     # misaligned outputs
        assert lr_call(inp.vecs, good, good, good, lo, ro + 8) == -1
        assert lr_call(inp.vecs, good, good, good, lo, lo) == -1                         # l_x over r_x
        assert lr_call(inp.vecs, good, good, good, lo, lo + 32 * (N - 1)) == -1
        for p, ln in zip(inp.ptrs, inp.lens):                                            # an output over an input
            assert lr_call(inp.vecs, good, good, good, p + 32 * (ln - 1), ro) == -1
            assert lr_call(inp.vecs, good, good, good, lo, p - 32 * (N - 1)) == -1
            assert lr_call(inp.vecs, good, good, good, p - 32, ro) == -1                 # the input nested inside the output
            assert lr_call(inp.vecs, good, good, good, lo, p - 32) == -1
        assert (t_out == SENT).all() and (tx_out == SENT).all()
        assert np.array_equal(out.read(), out.expected(c, [None, None]))
        assert inp.unchanged()
    finally:
        out.free()
        inp.free()


# ------------------------------------------------------------------------------------------- the a / b fold
def _fold_ref(a, b, x, r):
    m = len(a) // 2
    xi = pow(x, -1, r)
    a2 = [(x * a[j] + xi * a[j + m]) % r for j in range(m)]
    b2 = [(xi * b[j] + x * b[j + m]) % r for j in range(m)]
    h = m // 2
    return a2, b2, (ref.dot(a2[:h], b2[h:], r), ref.dot(a2[h:], b2[:h], r))


@pytest.mark.parametrize("n", [2, 4, 8, 128, 1024])
@pytest.mark.parametrize("curve", CURVES)
def test_ipa_fold_ab(ctx, curve, n):
    c = get_curve(curve)
    r = c.r
    a, _ = _values(c, n, n)
    b, _ = _values(c, n, n + 1)
    b.reverse()
    x = r - 1 if n in (4, 128) else rand_fr(r, 1, n)[0]
    a2, b2, cs_ref = _fold_ref(a, b, x, r)
    m = n // 2
    buf = Bufs(ctx, 2, n)
    try:
        for want_c in (True, False):
            buf.fill(c, [a, b])
            cs = ctx.fr_ipa_fold_ab_dev(c, buf.ptr(0), buf.ptr(1), n, codec.fr_mont(x, c), want_c=want_c)
            assert np.array_equal(buf.read(), buf.expected(c, [a2 + a[m:], b2 + b[m:]]))       # the high halves are unchanged
            if want_c and m >= 2:
                assert (codec.fr_int(cs[0], c), codec.fr_int(cs[1], c)) == cs_ref
            else:
                assert cs is None
        if m == 1:                                                 # c_out_host is not written when there is nothing to compute
            c_out = np.full((2, 4), SENT, dtype=np.uint64)
            buf.fill(c, [a, b])
            V = _lib.C.c_void_p
            xm = codec.fr_mont(x, c)
            assert ctx.lib.zkp_fr_ipa_fold_ab_dev(ctx.h, c.cid, V(buf.ptr(0)), V(buf.ptr(1)), n, V(xm.ctypes.data), V(c_out.ctypes.data)) == 0
            assert (c_out == SENT).all()
    finally:
        buf.free()


def test_ipa_fold_ab_two_pairs_per_thread(ctx):
    """n = 8 T_MAX: m / 2 = 2 T_MAX pairs, the first power of two at which a thread owns a second pair.  The vectors have period
    PERIOD, and so have the folded ones: the expectation is formed per residue."""
    c = get_curve("bls12_381")
    r = c.r
    n = 8 * T_MAX
    m, h = n // 2, n // 4
    assert h == 2 * T_MAX
    base_a, base_b = rand_fr(r, PERIOD, 1), rand_fr(r, PERIOD, 2)
    base_a[0], base_b[0], base_a[1] = 0, r - 1, r - 1
    x = rand_fr(r, 1, 3)[0]
    xi = pow(x, -1, r)
    idx = np.arange(n) % PERIOD
    wa, wb = codec.fr_to_mont(base_a, c), codec.fr_to_mont(base_b, c)
    host = np.full((2, n + 2, 4), SENT, dtype=np.uint64)
    host[0, 1:-1], host[1, 1:-1] = wa[idx], wb[idx]
    dev = ctx.to_device(host)
    try:
        cs = ctx.fr_ipa_fold_ab_dev(c, dev + 32, dev + 32 * (n + 3), n, codec.fr_mont(x, c))
        # a'[j] = x a[j] + x^-1 a[j + m] depends on j mod PERIOD only
        a2 = [(x * base_a[k] + xi * base_a[(k + m) % PERIOD]) % r for k in range(PERIOD)]
        b2 = [(xi * base_b[k] + x * base_b[(k + m) % PERIOD]) % r for k in range(PERIOD)]
        want = host.copy()
        want[0, 1:1 + m], want[1, 1:1 + m] = codec.fr_to_mont(a2, c)[idx[:m]], codec.fr_to_mont(b2, c)[idx[:m]]
        got = np.zeros_like(host)
        ctx.d2h(got, dev)
        assert np.array_equal(got, want)
        count = [(h - k + PERIOD - 1) // PERIOD for k in range(PERIOD)]                 # indices j < h with j mod PERIOD == k
        c_l = sum(count[k] * a2[k] * b2[(k + h) % PERIOD] for k in range(PERIOD)) % r
        c_r = sum(count[k] * a2[(k + h) % PERIOD] * b2[k] for k in range(PERIOD)) % r
        assert (codec.fr_int(cs[0], c), codec.fr_int(cs[1], c)) == (c_l, c_r)
    finally:
        ctx.dev_free(dev)


@pytest.mark.parametrize("curve", CURVES)
def test_ipa_fold_ab_chain_matches_dot_batch(ctx, curve):
    c = get_curve(curve)
    r = c.r
    n = 64
    a, _ = _values(c, n, 40)
    b, _ = _values(c, n, 41)
    buf = Bufs(ctx, 2, n)
    try:
        buf.fill(c, [a, b])
        pa, pb = buf.ptr(0), buf.ptr(1)
        length = n
        for k, x in enumerate(rand_fr(r, 6, 42)):
            cs = ctx.fr_ipa_fold_ab_dev(c, pa, pb, length, codec.fr_mont(x, c))
            a2, b2, cs_ref = _fold_ref(a[:length], b[:length], x, r)
            length //= 2
            a[:length], b[:length] = a2, b2
            if length >= 2:
                h = length // 2
                dots = ctx.fr_dot_batch_dev(c, [pa, pa + 32 * h], [pb + 32 * h, pb], [h, h])
                assert np.array_equal(cs, dots), k
                assert (codec.fr_int(cs[0], c), codec.fr_int(cs[1], c)) == cs_ref
            else:
                assert cs is None
        assert length == 1
        assert np.array_equal(buf.read(), buf.expected(c, [a, b]))
    finally:
        buf.free()


def test_ipa_fold_ab_argument_rules(ctx):
    c = get_curve("bn254")
    n = 8
    a, _ = _values(c, n, 1)
    b, _ = _values(c, n, 2)
    buf = Bufs(ctx, 2, n)
    good, zero, rr = codec.fr_mont(77, c), codec.fr_mont(0, c), codec.ints_to_limbs([c.r], 4)[0]
    try:
        buf.fill(c, [a, b])
        pa, pb = buf.ptr(0), buf.ptr(1)
        _bad_arg(lambda: ctx.fr_ipa_fold_ab_dev(c, pa, pb, n, zero))
        _bad_arg(lambda: ctx.fr_ipa_fold_ab_dev(c, pa, pb, n, rr))
        for bad_n in (0, 1, 6, 1 << 29):
            _bad_arg(lambda: ctx.fr_ipa_fold_ab_dev(c, pa, pb, bad_n, good))
        _bad_arg(lambda: ctx.fr_ipa_fold_ab_dev(c, pa + 8, pb, 4, good))
        _bad_arg(lambda: ctx.fr_ipa_fold_ab_dev(c, pa, pb + 8, 4, good))
        _bad_arg(lambda: ctx.fr_ipa_fold_ab_dev(c, pa, pa + 32 * 2, 4, good))          # a over b
        assert np.array_equal(buf.read(), buf.expected(c, [a, b]))
    finally:
        buf.free()


# ------------------------------------------------------------------------------------------- whole proofs
def _case(curve, N):
    if N == 16:
        return mini(curve), [10]
    n, n_w = {1: (1, 1), 4: (3, 2), 8: (2, 5), 32: (20, 7)}[N]
    cs = random_circuit(curve, n, n_w, 1000 + N)
    return cs, cs.input_assignment[1:]


@pytest.mark.parametrize("N", [1, 4, 8, 16, 32])
@pytest.mark.parametrize("curve", CURVES)
def test_prove_equals_the_reference_and_verifies(ctx, curve, N):
    cs, public = _case(curve, N)
    assert 1 << (max(cs.num_constraints(), cs.num_aux) - 1).bit_length() == N
    ints, gens = generators(curve, N, 50 + N)
    rand = randomness(curve, cs, 60 + N)
    want = ref.prove(curve, cs, ints, rand, Challenger(curve))
    rands = iter(rand)
    for r1cs, rnd in ((cs, rand), (R1csInstance.from_cs(cs), lambda: next(rands))):     # explicit values, then a callable
        got = bulletproofs.prove(ctx, curve, r1cs, gens, rnd, Challenger(curve))
        assert_same_proof(got, want)
    assert len(got.L_vec) == N.bit_length() - 1                    # N = 1: an argument of zero rounds
    assert ref.verify(curve, cs, ints, got, public, Challenger(curve))


def test_mini_proof_equals_the_golden_file(ctx):
    cs, _, gens, rand = mini_setup(MINI_CURVE)
    got = bulletproofs.prove(ctx, MINI_CURVE, cs, gens, rand, Challenger(MINI_CURVE))
    assert proof_to_json(got, MINI_CURVE) == load_golden()


def test_prove_rejects_what_it_cannot_batch(ctx):
    cs = mini("bn254")
    _, gens = generators("bn254", 4, 1)
    with pytest.raises(ValueError):
        bulletproofs.prove(ctx, "bn254", cs, gens, randomness("bn254", cs, 1), Challenger("bn254"))     # 4 generators for N = 16
    big = R1csInstance("bn254", 1, 1, bulletproofs.MSM_SMALL_MAX_G1 + 1, None, None, None, z=[1, 2])
    with pytest.raises(ValueError, match="ZKP_MSM_SMALL_MAX_G1"):
        bulletproofs.prove(ctx, "bn254", big, gens, [], Challenger("bn254"))                            # N = 2^17: above the batch cap
