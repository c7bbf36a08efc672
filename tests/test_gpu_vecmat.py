"""zkp_fr_vecmat_dev on the device against Python integers: out[j] = sum_i l[i] m[i cols + j].  Sentinel-framed buffers, whole
buffers compared, inputs read back unchanged.  The shapes: one element, one row (a single launch), one column, rows on either side
of the row chunk (one / two chunks: the second launch), columns on either side of a workgroup's 64, and 2^10 x 2^10.  The
reference of the large shape is one integer matrix product in numpy object arithmetic per curve, shared by its tests."""
import functools
import random

import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec
from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.polycommit import VECMAT_ROW_CHUNK

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xDEADBEEFCAFEF00D
RC = VECMAT_ROW_CHUNK
SHAPES = [(1, 1), (1, 65), (65, 1), (2, 2), (3, 64), (RC - 1, 5), (RC, 5), (RC + 1, 5), (2 * RC + 1, 63)]


def _bad(fn, status=-1):
    with pytest.raises(_lib.ZkpError) as e:
        fn()
    assert e.value.status == status


def run(ctx, c, l_words, m_words, rows, cols):
    sent = np.full((1, 4), SENT, dtype=np.uint64)
    h_l, h_m = np.concatenate([sent, l_words, sent]), np.concatenate([sent, m_words, sent])
    h_o = np.full((cols + 2, 4), SENT, dtype=np.uint64)
    d_l, d_m, d_o = ctx.to_device(h_l), ctx.to_device(h_m), ctx.to_device(h_o)
    try:
        ctx.fr_vecmat_dev(c, d_l + 32, d_m + 32, rows, cols, d_o + 32)
        g_l, g_m, g_o = np.zeros_like(h_l), np.zeros_like(h_m), np.zeros_like(h_o)
        ctx.d2h(g_l, d_l)
        ctx.d2h(g_m, d_m)
        ctx.d2h(g_o, d_o)
    finally:
        for d in (d_l, d_m, d_o):
            ctx.dev_free(d)
    assert np.array_equal(g_l, h_l) and np.array_equal(g_m, h_m), "an input changed"
    assert (g_o[0] == SENT).all() and (g_o[-1] == SENT).all(), "a write outside out"
    return g_o[1:-1]


def check(ctx, curve, rows, cols, l, m):
    c = get_curve(curve)
    want = [sum(l[i] * m[i * cols + j] for i in range(rows)) % c.r for j in range(cols)]
    got = run(ctx, c, codec.fr_to_mont(l, c), codec.fr_to_mont(m, c), rows, cols)
    assert np.array_equal(got, codec.fr_to_mont(want, c)), (curve, rows, cols)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_small_shapes(ctx, curve, shape):
    rows, cols = shape
    r = get_curve(curve).r
    rng = random.Random(f"{curve} {shape}")
    check(ctx, curve, rows, cols, [rng.randrange(r) for _ in range(rows)], [rng.randrange(r) for _ in range(rows * cols)])
    check(ctx, curve, rows, cols, [r - 1] * rows, [r - 1] * (rows * cols))
    check(ctx, curve, rows, cols, [0] * rows, [rng.randrange(r) for _ in range(rows * cols)])
    check(ctx, curve, rows, cols, [rng.randrange(r) for _ in range(rows)], [0] * (rows * cols))


@functools.lru_cache(maxsize=None)
def large_case(curve):
    """2^10 x 2^10 random values and l^T M in Python integers (numpy object arrays: one exact integer matrix product)"""
    c = get_curve(curve)
    n = 1 << 10
    rng = random.Random("vecmat large " + curve)
    l = [rng.randrange(c.r) for _ in range(n)]
    m = [rng.randrange(c.r) for _ in range(n * n)]
    want = np.array(l, dtype=object) @ np.array(m, dtype=object).reshape(n, n)
    return l, m, [int(v) % c.r for v in want]


@pytest.mark.parametrize("curve", CURVES)
def test_2_10_by_2_10(ctx, curve):
    c = get_curve(curve)
    n = 1 << 10
    l, m, want = large_case(curve)
    got = run(ctx, c, codec.fr_to_mont(l, c), codec.fr_to_mont(m, c), n, n)
    assert np.array_equal(got, codec.fr_to_mont(want, c))
    rmax = codec.fr_to_mont([c.r - 1], c)
    got = run(ctx, c, np.repeat(rmax, n, axis=0), np.repeat(rmax, n * n, axis=0), n, n)       # r - 1 everywhere: n (r - 1)^2 = n
    assert np.array_equal(got, np.repeat(codec.fr_to_mont([n], c), n, axis=0))
    got = run(ctx, c, np.zeros((n, 4), dtype=np.uint64), codec.fr_to_mont(m, c), n, n)
    assert (got == 0).all()


@pytest.mark.parametrize("curve", CURVES)
def test_argument_rules_write_nothing(ctx, curve):
    c = get_curve(curve)
    rows, cols = 3, 4
    h = np.full((64, 4), SENT, dtype=np.uint64)
    h_m = codec.fr_to_mont(list(range(rows * cols)), c)
    d_l, d_m, d_o = ctx.to_device(h), ctx.to_device(h_m), ctx.to_device(h)
    try:
        f = lambda **kw: ctx.fr_vecmat_dev(c, kw.get("l", d_l), kw.get("m", d_m), kw.get("rows", rows), kw.get("cols", cols), kw.get("o", d_o))
        for name, p in (("l", d_l), ("m", d_m), ("o", d_o)):
            _bad(lambda: f(**{name: 0}))
            _bad(lambda: f(**{name: p + 8}))
        _bad(lambda: f(rows=0))
        _bad(lambda: f(cols=0))
        _bad(lambda: f(rows=(1 << 28) // cols + 1))
        _bad(lambda: f(o=d_l))                                       # out over l, inside l, over m
        _bad(lambda: f(o=d_l + 32))
        _bad(lambda: f(l=d_o + 32 * (cols - 1)))
        _bad(lambda: f(o=d_m + 32))
        got, got_m = np.zeros_like(h), np.zeros_like(h_m)
        for d in (d_l, d_o):
            ctx.d2h(got, d)
            assert np.array_equal(got, h), "a refused call wrote"
        ctx.d2h(got_m, d_m)
        assert np.array_equal(got_m, h_m)
    finally:
        for d in (d_l, d_m, d_o):
            ctx.dev_free(d)
