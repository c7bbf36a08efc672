"""GPU: the Fr vector and polynomial kernels of csrc/poly.hip at the sizes where their blocking changes the code that runs, through
the C ABI, bit-exact on Montgomery words against tests/poly_ref.py and plain Python integers (never against another kernel).

The sizes come from the constants of poly.hip: POLY_CHUNK = 32 coefficients per lane and 256 chunks per tile (8192 coefficients,
horner_fix_kernel from the second tile on), 256 tiles per group of horner_scan_body (2^21 coefficients, a carry from the second
group on), lanes = ceil(n / 32) of the batch inversion, 256 threads per workgroup of the element-wise kernels, SPMV_LONG = 128,
SPMV_CHUNK = 8192, the reduce grid of 256 workgroups, SPMV_LIST_CAP = SPMV_PART_CAP = 65536, and the 8-row and 4096-coefficient
switches of poly_vanishing_fold.  Every output has one sentinel element before and after it, checked after every call."""
import ctypes
import functools
import random

import numpy as np
import pytest

from ckb_zkp_amd import api, codec
from ckb_zkp_amd.params import get_curve
from tests import marlin_hostlist, poly_ref
from tests.util import TEST_FULL

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xABABABABABABABAB
BIG = 1 << 21                                                        # coefficients in one group of horner_scan_body


class Guarded:
    """n Fr elements in device memory with one sentinel element before and after; everything is a sentinel unless `fill` is given"""

    def __init__(self, ctx, n, fill=None):
        self.ctx, self.n = ctx, n
        self.host = np.full((n + 2, 4), SENT, dtype=np.uint64)
        if fill is not None:
            self.host[1:n + 1] = fill
        self.dev = ctx.to_device(self.host)
        self.ptr = self.dev + 32

    def read(self):
        got = np.zeros_like(self.host)
        self.ctx.d2h(got, self.dev)
        assert (got[0] == SENT).all() and (got[-1] == SENT).all(), "a sentinel was overwritten"
        return got[1:-1]

    def untouched(self):
        return np.array_equal(self.read(), self.host[1:-1])


@pytest.fixture
def mk(ctx):
    made = []

    def make(n, fill=None):
        made.append(Guarded(ctx, n, fill))
        return made[-1]

    yield make
    for g in made:
        ctx.dev_free(g.dev)


@pytest.fixture
def up(ctx):
    """plain uploads of read-only inputs that are not Fr vectors (CSR arrays, indices)"""
    made = []

    def upload(a):
        made.append(ctx.to_device(np.ascontiguousarray(a)))
        return made[-1]

    yield upload
    for d in made:
        ctx.dev_free(d)


def _words(c, n, seed):
    """n elements drawn directly as Montgomery words: any words below r are some element's Montgomery form"""
    rng = np.random.default_rng(seed)
    w = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    w[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)      # < 2^(bits - 1) < r
    return w


def _same(got, exp, what):
    assert got.shape == exp.shape, what
    if not np.array_equal(got, exp):
        bad = np.flatnonzero((got != exp).any(axis=-1))
        pytest.fail(f"{what}: {len(bad)} of {len(exp)} elements differ, the first at {bad[0]}, the last at {bad[-1]}")


def _mont(c, xs):
    return codec.fr_to_mont(xs, c).reshape(-1, 4)


# ------------------------------------------------------------------------------------------- evaluate / divide by (X - z)
# 8191 .. 3 * 8192 + 1: one tile, one full tile, a second tile of one chunk with one coefficient, two full tiles, a third tile,
# three tiles and one coefficient.  2^21, 2^21 + 1, 2^21 + 24581: horner_scan_body runs one full group of 256 tiles, a second group
# of one tile with one chunk, and a second group of four tiles whose last chunk is ragged.
HORNER = [(cu, n, "dense") for cu in CURVES for n in (8191, 8192, 8193, 16384, 16385, 3 * 8192 + 1)]
HORNER += [("bn254", n, "dense") for n in (BIG, BIG + 1, BIG + 24581)] + [("bls12_381", BIG + 1, "dense")]
HORNER += [(cu, n, kind) for cu in CURVES for n in (8193, BIG + 1) for kind in ("z=0", "z=1", "z=r-1", "p=0", "p=last", "p=top0")]
HORNER.sort(key=lambda t: (t[0], t[1]))                             # the cases that share a dense p follow each other


@functools.lru_cache(maxsize=1)
def _dense(curve, n):
    w = _words(get_curve(curve), n, n)
    w[5] = 0
    return w, codec.limbs_to_ints(w)


@pytest.mark.parametrize("curve,n,kind", HORNER, ids=lambda v: str(v))
def test_evaluate_and_div_linear(ctx, mk, curve, n, kind):
    """p(z) from both entry points and every coefficient of p / (X - z).  Besides a dense random p and a random z: z = 0, 1, r - 1;
    p = 0; p = X^(n-1), whose quotient X^(n-2) + z X^(n-3) + ... shows every tile's and group's power of z; p with its top tile
    zero."""
    c = get_curve(curve)
    r = c.r
    w, ints = _dense(curve, n)
    z = {"z=0": 0, "z=1": 1, "z=r-1": r - 1}.get(kind, random.Random(n).randrange(2, r - 1))
    if kind == "p=0":
        w, ints = np.zeros_like(w), [0] * n
    elif kind == "p=last":
        w = np.zeros_like(w)
        w[-1] = _mont(c, [1])[0]
        ints = [0] * (n - 1) + codec.limbs_to_ints(w[-1:])
    elif kind == "p=top0":
        w = w.copy()
        w[n - 8192:] = 0
        ints = ints[:n - 8192] + [0] * 8192
    q_exp, ev_exp = poly_ref.horner_words(ints, z, r)
    if kind == "p=last":
        assert q_exp[0] == ints[-1] * pow(z, n - 2, r) % r and q_exp[-1] == ints[-1]
    zm = codec.fr_to_mont([z], c)[0]
    p, q = mk(n, w), mk(n - 1)
    assert codec.limbs_to_ints(ctx.poly_evaluate(c, p.ptr, n, zm).reshape(1, 4))[0] == ev_exp, "zkp_poly_evaluate_dev"
    assert q.untouched()
    ev = ctx.poly_div_linear(c, p.ptr, n, zm, q.ptr)
    assert codec.limbs_to_ints(ev.reshape(1, 4))[0] == ev_exp, "zkp_poly_div_linear_dev"
    _same(q.read(), codec.ints_to_limbs(q_exp, 4), "quotient")
    assert p.untouched()


@pytest.mark.parametrize("curve", CURVES)
def test_evaluate_and_div_linear_without_a_quotient(ctx, mk, curve):
    """n = 0 and n = 1: the evaluation is 0 or p_0 and q is not written (it may be NULL)"""
    c = get_curve(curve)
    w = _words(c, 1, 1)
    p, q = mk(1, w), mk(1)
    zm = codec.fr_to_mont([random.Random(1).randrange(c.r)], c)[0]
    for n, want in ((0, [0] * 4), (1, w[0].tolist())):
        for p_dev in ([p.ptr, 0] if n == 0 else [p.ptr]):
            assert ctx.poly_evaluate(c, p_dev, n, zm).tolist() == want, n
            assert ctx.poly_div_linear(c, p_dev, n, zm, q.ptr).tolist() == want, n
            if p_dev:                                                # NULL and NULL is q == p, which is rejected
                assert ctx.poly_div_linear(c, p_dev, n, zm, 0).tolist() == want, n
        assert q.untouched() and p.untouched()


# ------------------------------------------------------------------------------------------- batch inversion
def _lanes(n):
    return (n + 31) // 32


ZEROS = {"none": lambda n: [], "all": lambda n: range(n),
         "lane": lambda n: range(_lanes(n) - 1, n, _lanes(n)),      # every element of the last lane: t, t + lanes, ...
         "first": lambda n: [0], "last": lambda n: [n - 1], "alternating": lambda n: range(0, n, 2)}


@functools.lru_cache(maxsize=None)
def _inv_base(curve, n):
    r = get_curve(curve).r
    rnd = random.Random(n)
    xs = [rnd.randrange(2, r - 1) for _ in range(n)]
    for i, v in ((0, r - 1), (1, 1), (3, r - 1), (n - 1, 1)):
        if i < n:
            xs[i] = v
    return xs, poly_ref.batch_inverse(xs, r)


@pytest.mark.parametrize("zeros", list(ZEROS))
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 8191, 8192, 8193, 20011])
@pytest.mark.parametrize("curve", CURVES)
def test_batch_inverse(ctx, mk, curve, n, zeros):
    c = get_curve(curve)
    xs, inv = (list(t) for t in _inv_base(curve, n))
    for i in ZEROS[zeros](n):
        xs[i] = inv[i] = 0
    v = mk(n, _mont(c, xs))
    ctx.fr_batch_inverse(c, v.ptr, n)
    _same(v.read(), _mont(c, inv), "inverses")
    ctx.fr_batch_inverse(c, v.ptr, n)
    _same(v.read(), v.host[1:-1], "the inverses of the inverses")


# ------------------------------------------------------------------------------------------- element-wise operations
OPS = {"mul": api.VEC_MUL, "add": api.VEC_ADD, "sub": api.VEC_SUB, "scale": api.VEC_SCALE, "axpy": api.VEC_AXPY, "addc": api.VEC_ADDC}
READS_B, READS_K = ("mul", "add", "sub", "axpy"), ("scale", "axpy", "addc")
VEC = [(cu, op, n, form) for cu in CURVES for n in (1, 255, 256, 257, 100003) for op in OPS
       for form in ("distinct", "out=a") + (("out=b",) if op in READS_B else ())]


@functools.lru_cache(maxsize=4)
def _vec_inputs(curve, n):
    r = get_curve(curve).r
    rnd = random.Random(n)
    a, b = ([rnd.randrange(r) for _ in range(n)] for _ in range(2))
    edge = [(x, y) for x in (0, 1, r - 1) for y in (0, 1, r - 1)]
    for i, (x, y) in enumerate(edge[-n:] if n < len(edge) else edge):     # n = 1: (r - 1, r - 1)
        a[i], b[i] = x, y
    return a, b, rnd.randrange(2, r - 1)


@functools.lru_cache(maxsize=8)
def _vec_expected(curve, n, op, k):
    c = get_curve(curve)
    a, b, _ = _vec_inputs(curve, n)
    f = {"mul": lambda x, y: x * y, "add": lambda x, y: x + y, "sub": lambda x, y: x - y, "scale": lambda x, y: k * x,
         "axpy": lambda x, y: x + k * y, "addc": lambda x, y: x + k}[op]
    return _mont(c, [f(x, y) % c.r for x, y in zip(a, b)])


@pytest.mark.parametrize("curve,op,n,form", VEC, ids=lambda v: str(v))
def test_vec_op(ctx, mk, curve, op, n, form):
    """all six operations with out apart from the inputs, out == a, and out == b where b is read (include/zkp_accel.h: out may
    alias a or b); k = 0, 1, r - 1 and a random element where k is read"""
    c = get_curve(curve)
    a_int, b_int, k_rand = _vec_inputs(curve, n)
    am, bm = _mont(c, a_int), _mont(c, b_int)
    for k in ((0, 1, c.r - 1, k_rand) if op in READS_K else (None,)):
        a, b = mk(n, am), mk(n, bm)
        out = {"distinct": mk(n), "out=a": a, "out=b": b}[form]
        ctx.fr_vec_op(c, OPS[op], a.ptr, b.ptr if op in READS_B else None, out.ptr, n, None if k is None else codec.fr_to_mont([k], c)[0])
        _same(out.read(), _vec_expected(curve, n, op, k), f"k = {k}")
        assert (out is a or a.untouched()) and (out is b or b.untouched()), k


# ------------------------------------------------------------------------------------------- sparse matrix-vector product
def _spmv(ctx, mk, up, c, row_ptr, col, coeff_words, x_words, timing=None):
    nrows = len(row_ptr) - 1
    d_rp, d_col = up(np.asarray(row_ptr, dtype=np.uint32)), up(np.asarray(col, dtype=np.uint32))
    d_cf, x, out = up(coeff_words), mk(len(x_words), x_words), mk(nrows)
    runs = []
    for _ in range(1 if timing is None else 2):
        ctx.h2d(out.dev, out.host)
        ctx.sync()
        ctx.timer_start()
        ctx.fr_spmv(c, d_rp, d_col, d_cf, nrows, x.ptr, out.ptr)
        ms = ctx.timer_stop_ms()
        if timing is not None:
            timing.append(ms)
        runs.append(out.read())
        assert x.untouched()
    return runs


def _spmv_python(c, lens, seed, ncols=300):
    """rows of the given lengths with repeated columns, coefficients from {0, 1, r - 1, random}, x with 0, r - 1 and 1; the
    expectation is a Python-integer loop"""
    r = c.r
    rnd = random.Random(seed)
    x = [rnd.randrange(r) for _ in range(ncols)]
    x[0], x[1], x[2] = 0, r - 1, 1
    rows = []
    for ln in lens:
        row = [(rnd.choice([0, 1, r - 1, rnd.randrange(r)]), rnd.randrange(ncols)) for _ in range(ln)]
        if ln >= 2:
            row[1] = (row[1][0], row[0][1])                          # a repeated column in every row
        if ln >= 4:
            row[2], row[3] = (r - 1, 1), (rnd.randrange(r), 0)       # (r - 1) * (r - 1) and a product with 0
        rows.append(row)
    row_ptr = [0]
    for row in rows:
        row_ptr.append(row_ptr[-1] + len(row))
    flat = [t for row in rows for t in row]
    exp = [sum(cf * x[j] for cf, j in row) % r for row in rows]
    return row_ptr, [j for _, j in flat], _mont(c, [cf for cf, _ in flat]), _mont(c, x), _mont(c, exp)


@pytest.mark.parametrize("curve", CURVES)
def test_spmv_row_length_boundaries(ctx, mk, up, curve):
    """rows of 0, 1, 127, 128 terms (lane loop), 129 (the shortest long row), 8191, 8192 (one chunk), 8193 (a second chunk of one
    term), 16384, 16385 terms; long rows first and last"""
    c = get_curve(curve)
    lens = [16385, 0, 1, 127, 128, 129, 8191, 8192, 0, 16384, 8193]
    row_ptr, col, cf, x, exp = _spmv_python(c, lens, 1)
    _same(_spmv(ctx, mk, up, c, row_ptr, col, cf, x)[0], exp, "rows")


@pytest.mark.parametrize("curve", CURVES)
def test_spmv_more_long_rows_than_reduce_workgroups(ctx, mk, up, curve):
    """600 rows of 129 terms: each of the 256 reduce workgroups takes two or three rows, and workgroup 0 of the partial kernel runs
    the workgroup sum 600 times in a row on the same LDS"""
    c = get_curve(curve)
    row_ptr, col, cf, x, exp = _spmv_python(c, [129] * 600, 2)
    _same(_spmv(ctx, mk, up, c, row_ptr, col, cf, x)[0], exp, "rows")


@pytest.mark.skipif(not TEST_FULL, reason="ZKP_TEST_FULL=0: SPMV_LIST_CAP and SPMV_PART_CAP are compile-time constants (65536); no smaller "
                                          "matrix than this one of 10 M terms reaches either fall-back")
def test_spmv_list_and_partial_caps(ctx, mk, up, capsys):
    """65 636 long rows, 200 of them with two chunks, and 300 short rows in between.  Whichever 65 536 long rows get a list slot, at
    least 100 two-chunk rows are among them, so their partial slots exceed SPMV_PART_CAP and the last listed rows are summed whole
    by their reduce workgroup; the 100 long rows without a list slot are summed by their lane.  The list order comes from atomics,
    so two runs overflow on different rows: both must match.  Coefficients are indexed from a table of {1, -1, 2, 3}, x is small,
    the expectation is the exact int64 sum of tests/poly_ref.py."""
    c = get_curve("bn254")
    rng = np.random.default_rng(65636)
    n_long, n_short, ncols = 65636, 300, 4096
    long_lens = np.full(n_long, 129, dtype=np.int64)
    # The two-chunk rows lie together where a list in row order runs out of partial slots (65 235 one-chunk rows before them, a hundred
    # after them), so that the row that does not fit is likely to be one of them and leaves the last slot free for the one-chunk rows
    # listed after it: the only order in which "does not fit from here on" differs from "does not fit".  The counting argument above
    # does not depend on where they lie.
    long_lens[65235:65435] = 8193
    is_short = np.zeros(n_long + n_short, dtype=bool)
    is_short[rng.choice(n_long + n_short, size=n_short, replace=False)] = True
    lens = np.empty(n_long + n_short, dtype=np.int64)
    lens[is_short], lens[~is_short] = rng.choice([0, 1, 5, 128], size=n_short), long_lens
    row_ptr = np.concatenate([[0], np.cumsum(lens)])
    nnz = int(row_ptr[-1])
    assert nnz < 1 << 24 and (lens > 128).sum() == n_long
    col = rng.integers(0, ncols, size=nnz, dtype=np.uint32)
    sel = rng.integers(0, 4, size=nnz, dtype=np.uint8)
    x_small = rng.integers(-1000, 1001, size=ncols)
    x_small[:3] = [0, -1, 1]
    exp = _mont(c, poly_ref.spmv_small_int(row_ptr, col, np.array([1, -1, 2, 3])[sel], x_small, c.r))
    timing = []
    runs = _spmv(ctx, mk, up, c, row_ptr, col, _mont(c, [1, -1, 2, 3])[sel], _mont(c, [int(v) for v in x_small]), timing)
    with capsys.disabled():
        print(f"\n[spmv caps] {nnz} terms, device time of the two calls: {timing[0]:.1f} ms, {timing[1]:.1f} ms")
    _same(runs[0], exp, "first run")
    _same(runs[1], exp, "second run")


# ------------------------------------------------------------------------------------------- divide by X^n - 1
# n = 64: 8 rows (replay only), 8 rows + 1 coefficient and 9 rows (two blocks of 8 rows), 9 rows + 1, 81 rows + 5 (blocks of 10 rows:
# the square root rounds up); n = 1: 4096 coefficients (strided sums), 4097 (division by X - 1); fewer coefficients than n; none
FOLD = [(ln, n, "q,rem") for ln, n in ((512, 64), (513, 64), (576, 64), (577, 64), (81 * 64 + 5, 64), (4096, 1), (4097, 1), (63, 64),
                                       (0, 4), (5000, 1))]
FOLD += [(ln, n, mode) for ln, n in ((5000, 1), (577, 64)) for mode in ("q", "rem")]


@pytest.mark.parametrize("length,n,mode", FOLD, ids=lambda v: str(v))
@pytest.mark.parametrize("curve", CURVES)
def test_divide_by_vanishing(ctx, mk, curve, length, n, mode):
    c = get_curve(curve)
    rnd = random.Random(length + n)
    p_int = [rnd.randrange(c.r) for _ in range(length)]
    eq, er = marlin_hostlist.divide_by_vanishing(p_int, n, c.r)      # trimmed lists
    nq = max(length - n, 0)
    p, q, rem = mk(length, _mont(c, p_int) if length else None), mk(nq), mk(n)
    ctx.poly_divide_by_vanishing(c, p.ptr, length, n, q.ptr if "q" in mode else None, rem.ptr if "rem" in mode else None)
    if "q" in mode:
        _same(q.read(), _mont(c, eq + [0] * (nq - len(eq))), "quotient")
    else:
        assert q.untouched()
    if "rem" in mode:
        _same(rem.read(), _mont(c, er + [0] * (n - len(er))), "remainder")
    else:
        assert rem.untouched()
    assert p.untouched()


# ------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("case", ["all -1", "all last", "repeats"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gather(ctx, mk, up, n, case):
    m = 9
    src = np.frombuffer(np.random.default_rng(n).bytes(32 * m), dtype=np.uint64).reshape(m, 4)     # any bits: the kernel only copies
    idx = {"all -1": np.full(n, -1), "all last": np.full(n, m - 1),
           "repeats": np.random.default_rng(n + 1).choice([0, 0, 0, 3, m - 1, -1], size=n)}[case].astype(np.int32)
    table, out = mk(m, src), mk(n)
    ctx.fr_gather(table.ptr, up(idx), n, out.ptr)
    _same(out.read(), np.where(idx[:, None] < 0, np.uint64(0), src[np.maximum(idx, 0)]), case)
    assert table.untouched()


# ------------------------------------------------------------------------------------------- argument rules
@pytest.mark.parametrize("curve", CURVES)
def test_rejected_calls_leave_everything_untouched(ctx, mk, up, curve):
    """the NULL, q == p and unknown-curve cases of the seven entry points return ZKP_ERR_BAD_ARG (-1) / ZKP_ERR_UNSUPPORTED_CURVE (-2)
    and write nothing, on the device or on the host"""
    c = get_curve(curve)
    n, cid, lib, h = 40, c.cid, ctx.lib, ctx.h
    a, b, out, q = mk(n), mk(n), mk(n), mk(n)
    d_idx = up(np.zeros(n, dtype=np.int32))
    d_rp, d_col = up(np.arange(n + 1, dtype=np.uint32)), up(np.zeros(n, dtype=np.uint32))
    k = codec.fr_to_mont([5], c)[0]
    ev = np.full(4, SENT, dtype=np.uint64)
    V = ctypes.c_void_p
    kp, evp = V(k.ctypes.data), V(ev.ctypes.data)
    A, B, O, Q = a.ptr, b.ptr, out.ptr, q.ptr
    bad_arg = [
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_ADD, None, B, None, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_ADD, A, B, None, None, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_MUL, A, None, None, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_ADD, A, None, None, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_SUB, A, None, None, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_AXPY, A, None, kp, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_AXPY, A, B, None, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_SCALE, A, None, None, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, api.VEC_ADDC, A, None, None, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, 6, A, B, kp, O, n),
        lambda: lib.zkp_fr_vec_op_dev(h, cid, -1, A, B, kp, O, n),
        lambda: lib.zkp_fr_spmv_dev(h, cid, None, d_col, A, n, B, O),
        lambda: lib.zkp_fr_spmv_dev(h, cid, d_rp, d_col, A, n, None, O),
        lambda: lib.zkp_fr_spmv_dev(h, cid, d_rp, d_col, A, n, B, None),
        lambda: lib.zkp_fr_gather_dev(h, None, d_idx, n, O),
        lambda: lib.zkp_fr_gather_dev(h, A, None, n, O),
        lambda: lib.zkp_fr_gather_dev(h, A, d_idx, n, None),
        lambda: lib.zkp_poly_divide_by_vanishing_dev(h, cid, None, n, 8, Q, O),
        lambda: lib.zkp_poly_divide_by_vanishing_dev(h, cid, A, n, 0, Q, O),
        lambda: lib.zkp_fr_batch_inverse_dev(h, cid, None, n),
        lambda: lib.zkp_poly_evaluate_dev(h, cid, None, n, kp, evp),
        lambda: lib.zkp_poly_evaluate_dev(h, cid, A, n, None, evp),
        lambda: lib.zkp_poly_evaluate_dev(h, cid, A, n, kp, None),
        lambda: lib.zkp_poly_div_linear_dev(h, cid, None, n, kp, Q, evp),
        lambda: lib.zkp_poly_div_linear_dev(h, cid, A, n, None, Q, evp),
        lambda: lib.zkp_poly_div_linear_dev(h, cid, A, n, kp, None, evp),
        lambda: lib.zkp_poly_div_linear_dev(h, cid, A, n, kp, A, evp),                  # q == p
    ]
    bad_curve = [
        lambda: lib.zkp_fr_vec_op_dev(h, 7, api.VEC_AXPY, A, B, kp, O, n),
        lambda: lib.zkp_fr_spmv_dev(h, 7, d_rp, d_col, A, n, B, O),
        lambda: lib.zkp_poly_divide_by_vanishing_dev(h, 7, A, n, 8, Q, O),
        lambda: lib.zkp_poly_divide_by_vanishing_dev(h, 7, A, n, 1, Q, O),
        lambda: lib.zkp_fr_batch_inverse_dev(h, 7, A, n),
        lambda: lib.zkp_poly_evaluate_dev(h, 7, A, n, kp, evp),
        lambda: lib.zkp_poly_div_linear_dev(h, 7, A, n, kp, Q, evp),
    ]
    for i, call in enumerate(bad_arg):
        assert call() == -1, i
    for i, call in enumerate(bad_curve):
        assert call() == -2, i
    ctx.sync()
    assert all(g.untouched() for g in (a, b, out, q)) and (ev == SENT).all()
    # the context still works: a good call of each kind of output
    xs = list(range(1, n + 1))
    ctx.h2d(a.ptr, _mont(c, xs))
    ctx.h2d(b.ptr, _mont(c, [c.r - 1] * n))
    ctx.fr_vec_op(c, api.VEC_ADD, a.ptr, b.ptr, out.ptr, n)
    _same(out.read(), _mont(c, [x - 1 for x in xs]), "a + (r - 1)")
    assert lib.zkp_poly_div_linear_dev(h, cid, A, n, kp, Q, evp) == 0
    q_exp, ev_exp = poly_ref.horner_words(codec.limbs_to_ints(_mont(c, xs)), 5, c.r)
    assert codec.limbs_to_ints(ev.reshape(1, 4))[0] == ev_exp
    _same(q.read()[:n - 1], codec.ints_to_limbs(q_exp, 4), "quotient")
    assert (q.read()[n - 1] == SENT).all()
