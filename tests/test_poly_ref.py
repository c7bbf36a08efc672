"""CPU: the reference helpers of tests/poly_ref.py, which the GPU cases of tests/test_gpu_poly_edges.py rest on, against the
oracle's own polynomial code and plain Python-integer loops."""
import random

import numpy as np
import pytest

from ckb_zkp_amd import codec
from ckb_zkp_amd.params import get_curve
from oracle.pyref import kzg10 as okzg
from tests import poly_ref

CURVES = ["bn254", "bls12_381"]


@pytest.mark.parametrize("n", [1, 2, 33, 1000])
@pytest.mark.parametrize("curve", CURVES)
def test_horner_words_equals_the_oracle_after_conversion(curve, n):
    c = get_curve(curve)
    rnd = random.Random(n)
    p = [rnd.randrange(c.r) for _ in range(n)]
    words = codec.limbs_to_ints(codec.fr_to_mont(p, c))
    for z in (0, 1, c.r - 1, rnd.randrange(c.r)):
        q, ev = poly_ref.horner_words(words, z, c.r)
        assert all(0 <= w < c.r for w in q) and len(q) == n - 1
        assert codec.fr_from_mont(codec.ints_to_limbs([ev], 4), c)[0] == okzg.evaluate(p, z, c.r), z
        if n > 1:
            assert codec.fr_from_mont(codec.ints_to_limbs(q, 4), c) == okzg.divide_by_linear(p, z, c.r), z
    assert poly_ref.horner_words([], 5, c.r) == ([], 0)


@pytest.mark.parametrize("curve", CURVES)
def test_batch_inverse_keeps_zeros(curve):
    r = get_curve(curve).r
    rnd = random.Random(5)
    xs = [0, 1, r - 1, 2, 0] + [rnd.randrange(r) for _ in range(50)] + [0]
    inv = poly_ref.batch_inverse(xs, r)
    assert [x * y % r for x, y in zip(xs, inv)] == [1 if x else 0 for x in xs]
    assert inv[1] == 1 and inv[2] == r - 1 and poly_ref.batch_inverse(inv, r) == xs
    assert poly_ref.batch_inverse([], r) == [] and poly_ref.batch_inverse([0, 0], r) == [0, 0]


@pytest.mark.parametrize("curve", CURVES)
def test_spmv_small_int_equals_a_python_loop(curve):
    r = get_curve(curve).r
    rng = np.random.default_rng(9)
    nrows, ncols = 500, 97
    lens = rng.choice([0, 0, 1, 2, 7, 130, 300], size=nrows)
    lens[0] = lens[1] = lens[-1] = 0                                 # empty rows first, twice in a row, and last
    lens[-2] = 9000
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    nnz = int(row_ptr[-1])
    col = rng.integers(0, ncols, size=nnz, dtype=np.uint32)
    cf = rng.integers(-(1 << 20) + 1, 1 << 20, size=nnz)
    x = rng.integers(-(1 << 20) + 1, 1 << 20, size=ncols)
    cf[:3], x[0], x[1] = [(1 << 20) - 1, -(1 << 20) + 1, 0], (1 << 20) - 1, -(1 << 20) + 1
    got = poly_ref.spmv_small_int(row_ptr, col, cf, x, r)
    want = [sum(int(cf[k]) * int(x[col[k]]) for k in range(row_ptr[i], row_ptr[i + 1])) % r for i in range(nrows)]
    assert got == want and any(w > r // 2 for w in want) and got[0] == got[1] == got[-1] == 0
    assert poly_ref.spmv_small_int([0, 0, 0], [], [], x, r) == [0, 0]                   # nothing but empty rows
    with pytest.raises(AssertionError):
        poly_ref.spmv_small_int([0, 1], [0], [1 << 20], x, r)
