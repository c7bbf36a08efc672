"""Sum-check provers on the device: the loops of `sum_check_proof_phase_one`, `sum_check_proof_phase_two` and
`sum_check_cubic_prover` (spartan/src/prover.rs:422-592, 594-723, 1442-1607) and the compute backbone of `r1cs_satisfied_prover`
(prover.rs:265-371), with every table resident on the device from upload to the last round.

Per round one zkp_fr_sumcheck_round_dev call binds the previous challenge into every table and returns g(0), g(2), (g(3)) of the
next round polynomial; g(1) = claim - g(0) and the coefficients are formed on the host.  A proof of v rounds is v + 1 calls: the
last one only binds and leaves the final values at element 0 of each table.

The reference's commitments of the round polynomials, their blinds and its merlin transcript are the caller's, as in ipa.py:
`next_challenge(coeffs)` receives the round polynomial's coefficients (canonical Python integers, constant term first, as the
reference's DensePolynomial) and returns the challenge x as an integer.  Claims, polynomials, challenges and final values are
canonical integers; tables are Montgomery Fr (4 x u64 per element) on the device and are bound IN PLACE."""
from __future__ import annotations

import numpy as np

from .api import SC_EQ_AB_MINUS_C, SC_PROD2, SC_PROD3, VEC_AXPY, VEC_SCALE
from .codec import fr_int, fr_mont
from .params import get_curve


def first_element(ctx, ptr: int, c) -> int:
    """element 0 of a DEVICE table as an integer: where a bound table leaves its final value"""
    a = np.zeros(4, dtype=np.uint64)
    ctx.d2h(a, ptr)
    return fr_int(a, c)


def cubic_coeffs(e0: int, e2: int, e3: int, claim: int, r: int) -> list:
    """[d, c, b, a] of the cubic through g(0) = e0, g(1) = claim - e0, g(2) = e2, g(3) = e3 (prover.rs:499-516)"""
    e1 = (claim - e0) % r
    a = (-e0 + 3 * e1 - 3 * e2 + e3) * pow(6, -1, r) % r
    b = (2 * e0 - 5 * e1 + 4 * e2 - e3) * pow(2, -1, r) % r
    return [e0 % r, (e1 - e0 - a - b) % r, b, a]


def quadratic_coeffs(e0: int, e2: int, claim: int, r: int) -> list:
    """[c, b, a] of the quadratic through g(0) = e0, g(1) = claim - e0, g(2) = e2 (prover.rs:646-655)"""
    e1 = (claim - e0) % r
    a = (e0 - 2 * e1 + e2) * pow(2, -1, r) % r
    return [e0 % r, (e1 - a - e0) % r, a]


def evaluate_poly(coeffs, x: int, r: int) -> int:
    """a round polynomial (constant term first) at x"""
    acc = 0
    for cf in reversed(coeffs):
        acc = (acc * x + cf) % r
    return acc


def _prove(ctx, c, kind, tables, n, claim, next_challenge, to_coeffs):
    """the round loop: to_coeffs(evals, claim) -> coefficients, evals = one tuple of integers per term"""
    r = c.r
    assert n >= 1 and n & (n - 1) == 0
    polys, rs = [], []
    length, x = n, None
    claim %= r
    for _ in range(n.bit_length() - 1):
        ev = ctx.fr_sumcheck_round_dev(c, kind, tables, length, bind=None if x is None else fr_mont(x, c))
        if x is not None:
            length //= 2
        coeffs = to_coeffs([tuple(fr_int(p, c) for p in term) for term in ev], claim)
        x = next_challenge(list(coeffs)) % r
        claim = evaluate_poly(coeffs, x, r)
        polys.append(coeffs)
        rs.append(x)
    if x is not None:
        ctx.fr_sumcheck_round_dev(c, kind, tables, length, bind=fr_mont(x, c), want_evals=False)
    return polys, rs


def prove_phase_one(ctx, curve, d_eq, d_a, d_b, d_c, n, claim, next_challenge):
    """sum_check_proof_phase_one: g = eq (a b - c) over DEVICE tables of n Fr.  Returns (polys, rx, (va, vb, vc, veq))."""
    c = get_curve(curve)
    polys, rx = _prove(ctx, c, SC_EQ_AB_MINUS_C, [d_eq, d_a, d_b, d_c], n, claim, next_challenge,
                       lambda ev, cl: cubic_coeffs(*ev[0], cl, c.r))
    return polys, rx, tuple(first_element(ctx, p, c) for p in (d_a, d_b, d_c, d_eq))


def prove_phase_two(ctx, curve, d_abc, d_z, n, claim, next_challenge):
    """sum_check_proof_phase_two: g = abc z over DEVICE tables of n Fr.  Returns (polys, ry, (vs, vz))."""
    c = get_curve(curve)
    polys, ry = _prove(ctx, c, SC_PROD2, [d_abc, d_z], n, claim, next_challenge, lambda ev, cl: quadratic_coeffs(*ev[0], cl, c.r))
    return polys, ry, tuple(first_element(ctx, p, c) for p in (d_abc, d_z))


def prove_cubic_batched(ctx, curve, par, c_par, seq, coeffs, n, claim, next_challenge):
    """sum_check_cubic_prover: sum_k coeffs[k] a_k b_k c_k, the `par` terms (a, b) sharing the table c_par, then the `seq` terms
    (a, b, c); coeffs: integers, one per term in that order.  c_par is bound once per round however many terms share it.
    Returns (polys, r, (a_par, b_par, c_par), (a_seq, b_seq, c_seq)): the final values in the reference's grouping."""
    c = get_curve(curve)
    r = c.r
    assert len(coeffs) == len(par) + len(seq)
    tables = [p for a, b in par for p in (a, b, c_par)] + [p for t in seq for p in t]

    def to_coeffs(ev, cl):
        s = [sum(e[p] * w for e, w in zip(ev, coeffs)) % r for p in range(3)]
        return cubic_coeffs(s[0], s[1], s[2], cl, r)

    polys, rs = _prove(ctx, c, SC_PROD3, tables, n, claim, next_challenge, to_coeffs)
    f = lambda p: first_element(ctx, p, c)                                # noqa: E731
    return (polys, rs, ([f(a) for a, _ in par], [f(b) for _, b in par], f(c_par) if par else None),
            ([f(a) for a, _, _ in seq], [f(b) for _, b, _ in seq], [f(t) for _, _, t in seq]))


def transpose_csr(csr, ncols: int):
    """(row_ptr, col, coeff) of M -> the CSR of M^T with ncols rows (host, numpy); entries of a column keep their row order"""
    row_ptr, col, coeff = (np.asarray(csr[0], dtype=np.uint32), np.asarray(csr[1], dtype=np.uint32),
                           np.ascontiguousarray(csr[2], dtype=np.uint64).reshape(-1, 4))
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.uint32), np.diff(row_ptr.astype(np.int64)))
    order = np.argsort(col, kind="stable")
    t_ptr = np.zeros(ncols + 1, dtype=np.uint32)
    t_ptr[1:] = np.cumsum(np.bincount(col, minlength=ncols))
    return t_ptr, rows[order], np.ascontiguousarray(coeff[order])


def r1cs_sumcheck(ctx, curve, csr_a, csr_b, csr_c, z, tau, challenge_1, abc_challenges, challenge_2):
    """The sum-checks of r1cs_satisfied_prover (prover.rs:265-371) without its commitments.
    csr_*: (row_ptr, col, coeff) host arrays of the 2^s-row R1CS matrices, coeff Montgomery; the column indices address z as the
    reference lays it out (aux first, inputs from len(z) / 2) and arrive already mapped.  z: (2^t, 4) Montgomery.
    tau: s integers.  challenge_1 / challenge_2: next_challenge of the two phases.  abc_challenges: (r_a, r_b, r_c), or a function
    of (va, vb, vc, veq) that returns them.
    Returns (polys_1, rx, (va, vb, vc, veq), polys_2, ry, (vs, vz))."""
    c = get_curve(curve)
    r = c.r
    z = np.ascontiguousarray(z, dtype=np.uint64).reshape(-1, 4)
    nz = z.shape[0]
    rows = len(csr_a[0]) - 1
    assert rows >= 1 and rows & (rows - 1) == 0 and nz & (nz - 1) == 0 and len(tau) == rows.bit_length() - 1
    bufs = []

    def up(arr):
        d = ctx.to_device(np.ascontiguousarray(arr))
        bufs.append(d)
        return d

    def alloc(nbytes):
        d = ctx.dev_alloc(nbytes)
        bufs.append(d)
        return d

    def up_csr(m):
        return (up(np.asarray(m[0], dtype=np.uint32)), up(np.asarray(m[1], dtype=np.uint32)),
                up(np.ascontiguousarray(m[2], dtype=np.uint64).reshape(-1, 4)))

    try:
        dz = up(z)
        # Az, Bz, Cz and eq(tau), then phase one
        d_abc = []
        for m in (csr_a, csr_b, csr_c):
            assert len(m[0]) - 1 == rows
            out = alloc(32 * rows)
            if len(m[1]):
                ctx.fr_spmv(c, *up_csr(m), rows, dz, out)
            else:
                ctx.dev_zero(out, 32 * rows)
            d_abc.append(out)
        d_eq = alloc(32 * rows)
        ctx.fr_eq_evals_dev(c, np.stack([fr_mont(t, c) for t in tau]).reshape(-1, 4) if len(tau) else np.zeros((0, 4), np.uint64), d_eq)
        polys_1, rx, vals = prove_phase_one(ctx, c, d_eq, *d_abc, rows, 0, challenge_1)
        va, vb, vc, _ = vals
        r_a, r_b, r_c = abc_challenges(*vals) if callable(abc_challenges) else abc_challenges
        # eq(rx), the three column products, their combination, then phase two against z
        ctx.fr_eq_evals_dev(c, np.stack([fr_mont(t, c) for t in rx]).reshape(-1, 4) if rx else np.zeros((0, 4), np.uint64), d_eq)
        d_cols = []
        for m in (csr_a, csr_b, csr_c):
            out = alloc(32 * nz)
            if len(m[1]):
                ctx.fr_spmv(c, *up_csr(transpose_csr(m, nz)), nz, d_eq, out)
            else:
                ctx.dev_zero(out, 32 * nz)
            d_cols.append(out)
        d_ev = d_cols[0]
        ctx.fr_vec_op(c, VEC_SCALE, d_cols[0], None, d_ev, nz, fr_mont(r_a, c))
        ctx.fr_vec_op(c, VEC_AXPY, d_ev, d_cols[1], d_ev, nz, fr_mont(r_b, c))
        ctx.fr_vec_op(c, VEC_AXPY, d_ev, d_cols[2], d_ev, nz, fr_mont(r_c, c))
        claim_2 = (r_a * va + r_b * vb + r_c * vc) % r
        polys_2, ry, vals_2 = prove_phase_two(ctx, c, d_ev, dz, nz, claim_2, challenge_2)
        return polys_1, rx, vals, polys_2, ry, vals_2
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
