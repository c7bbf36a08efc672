"""Plain references for the Fr vector / polynomial kernels of csrc/poly.hip: Python integers, and exact numpy integers where a
case is too large for a Python loop.  Nothing here calls the library; tests/test_poly_ref.py pins these helpers on the CPU."""
import numpy as np


def horner_words(p_words, z_int, r):
    """(q_words, eval_word) of p / (X - z) and p(z), on the MONTGOMERY words of p taken as integers, with z canonical.

    p(z) R = sum_j (p_j R) z^j is linear in p, so Horner's rule over the words p_j R mod r with the canonical z yields the
    Montgomery words of every quotient coefficient and of the evaluation: no conversion pass for the 2^21-coefficient cases.
    q has len(p) - 1 words (none for len(p) <= 1); the evaluation of the empty polynomial is 0."""
    n = len(p_words)
    q = [0] * max(n - 1, 0)
    acc = 0
    for i in range(n - 1, 0, -1):
        acc = (acc * z_int + p_words[i]) % r
        q[i - 1] = acc
    ev = (acc * z_int + p_words[0]) % r if n else 0
    return q, ev


def batch_inverse(xs, r):
    """ark_ff::fields::batch_inversion: every nonzero element inverted, zeros stay zero"""
    return [pow(x, -1, r) if x % r else 0 for x in xs]


def spmv_small_int(row_ptr, col, cf_small, x_small, r):
    """out[i] = sum_k cf[k] * x[col[k]] mod r over CSR arrays with SMALL signed integers (|cf|, |x| < 2^20), as Python integers.

    Every product is below 2^40 in magnitude and a row has fewer than 2^23 terms, so the int64 sums of np.add.reduceat are exact.
    reduceat gives an empty row the element at its start index (and rejects a start index at the very end), so the empty rows are
    left out of the call and set to zero explicitly."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    cf = np.asarray(cf_small, dtype=np.int64)
    xs = np.asarray(x_small, dtype=np.int64)
    assert (np.abs(cf) < 1 << 20).all() and (np.abs(xs) < 1 << 20).all()
    lens = np.diff(row_ptr)
    assert (lens >= 0).all() and (lens < 1 << 23).all() and row_ptr[0] == 0 and row_ptr[-1] == len(cf)
    sums = np.zeros(len(lens), dtype=np.int64)
    full = np.flatnonzero(lens > 0)
    if len(full):
        prod = cf * xs[np.asarray(col, dtype=np.int64)]
        sums[full] = np.add.reduceat(prod, row_ptr[full])      # consecutive non-empty starts: each segment ends at the next start
    return [int(s) % r for s in sums]
