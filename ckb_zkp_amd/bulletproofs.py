"""Bulletproofs R1CS prover on the device: `create_random_proof` / `prove` (bulletproofs/src/arithmetic_circuit.rs:187-612) and
`inner_product_proof::prove` (inner_product_proof.rs:22-111) over G1.  The generators, the assignment and every Fr vector go to the
device once and stay there.

  * aL, aR, aO = A f, B f, C f (zkp_fr_spmv_dev over the CSR matrices); z_Q = z, z^2, ... (zkp_fr_powers_dev) and
    v = z_Q WV = (A_w^T + zn B_w^T + zn^2 C_w^T) z_Q with the transposes restricted to the witness columns (three zkp_fr_spmv_dev
    calls and one zkp_fr_lincomb_dev);
  * A_I, A_O, A_W, S: one zkp_msm_g1_var_batch_dev call; T_2 .. T_10 (without T_4): one call; IPP_P: one call;
  * t_2 .. t_10: zkp_fr_bp_t_coeffs_dev; l(x), r(x), t_x: zkp_fr_bp_lr_eval_dev.  l(X) and r(X) are never stored;
  * per IPA round one zkp_msm_g1_var_batch_dev call of six entries for L and R, zkp_g1_ipa_fold_dev for g (x^-1, x) and for h
    (x, x^-1), and one zkp_fr_ipa_fold_ab_dev, which also returns the next round's cL and cR.

The merlin transcript stays with the caller (the reference absorbs the dense constraint matrices, which is host work): `challenger`
supplies yz(A_I, A_O, A_W, S) -> (y, z), x([T_2, T_3, T_5 .. T_10]) -> x, x1(t_x, tau_x, mu, l_x, r_x) -> x_1 and ipa(L, R) -> x.
Points are (xy, inf): affine Montgomery words and the identity flag; scalars are Python integers; l_x and r_x are (N, 4) uint64
Montgomery arrays.  `rand` is the prover's randomness in the reference's order (sL, sR, the blindings of A_I, A_O, S and A_W,
tau_2, 3, 5 .. 10): a callable returning the next value, or a sequence of 2 max(n, n_w) + 12 integers.

The verifier does not run here; tests/bulletproofs_ref.py has one in Python integers."""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from .codec import fr_int, fr_mont, fr_to_mont
from .params import get_curve

BP_THREADS = 256        # csrc/bulletproofs.hpp: threads per workgroup of every pass
BP_MAX_GROUPS = 512     # workgroups of one pass: a thread owns a second index above BP_THREADS * BP_MAX_GROUPS
BP_SUM_GROUP = 3        # sums reduced over a workgroup at a time
MSM_SMALL_MAX_G1 = 1 << 16          # ZKP_MSM_SMALL_MAX_G1
T_DEGREES = (2, 3, 5, 6, 7, 8, 9, 10)


@dataclass
class Generators:
    """bulletproofs Generators: g_vec_N, h_vec_N as (N, w) affine Montgomery arrays, g, h, u as (w,) arrays (none the identity)"""
    g_vec: np.ndarray
    h_vec: np.ndarray
    g: np.ndarray
    h: np.ndarray
    u: np.ndarray


@dataclass
class Proof:
    """the reference's Proof: points as (xy, inf), scalars as integers, l_x / r_x as (N, 4) Montgomery arrays; T holds T_2, T_3,
    T_5 .. T_10; L_vec, R_vec, a, b are the fields of IPP"""
    A_I: tuple
    A_O: tuple
    A_W: tuple
    S: tuple
    T: list
    mu: int
    tau_x: int
    l_x: np.ndarray
    r_x: np.ndarray
    t_x: int
    IPP_P: tuple
    L_vec: list = field(default_factory=list)
    R_vec: list = field(default_factory=list)
    a: int = 0
    b: int = 0


def drawer(rand, total: int):
    """draw(count) -> the next `count` values of the prover's randomness: `rand` is a callable or a sequence of `total` integers"""
    if callable(rand):
        return lambda count: [int(rand()) for _ in range(count)]
    vals = [int(v) for v in rand]
    if len(vals) != total:
        raise ValueError(f"the prover draws {total} values")
    it = iter(vals)
    return lambda count: [next(it) for _ in range(count)]


def witness_transpose(csr, num_inputs: int, num_aux: int):
    """the CSR form of M^T restricted to the witness columns: row j is column num_inputs + j of M"""
    row_ptr, col, coeff = csr
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))
    keep = col >= num_inputs
    t_rows, t_cols, t_coeff = col[keep] - num_inputs, rows[keep], np.asarray(coeff, dtype=np.uint64).reshape(-1, 4)[keep]
    order = np.argsort(t_rows, kind="stable")
    t_ptr = np.zeros(num_aux + 1, dtype=np.uint32)
    t_ptr[1:] = np.cumsum(np.bincount(t_rows, minlength=num_aux))
    return t_ptr, t_cols[order].astype(np.uint32), np.ascontiguousarray(t_coeff[order])


def prove(ctx, curve, r1cs, gens: Generators, rand, challenger, stats: dict | None = None) -> Proof:
    """r1cs: an R1csInstance or ConstraintSystem with its assignment (the one input first).  n = constraints, n_w = aux variables,
    N = the next power of two of max(n, n_w); gens holds N generators per vector.  N above ZKP_MSM_SMALL_MAX_G1 (65536) raises
    ValueError: the commitments are batched small MSMs.  N == 1 gives an inner-product argument of zero rounds.
    stats (a dict) receives the host's wall seconds per stage (every call returns when its work is done)."""
    c = get_curve(curve)
    r = c.r
    n, k, n_w = r1cs.num_constraints(), r1cs.num_inputs, r1cs.num_aux
    f = r1cs.full_assignment()
    if f is None or len(f) != k + n_w:
        raise ValueError("the constraint system carries no assignment")
    if n < 1:
        raise ValueError("no constraints")
    n_max = max(n, n_w)
    N = 1 << (n_max - 1).bit_length()
    if N > MSM_SMALL_MAX_G1:
        raise ValueError(f"N = {N} exceeds ZKP_MSM_SMALL_MAX_G1 = {MSM_SMALL_MAX_G1}")
    g_vec, h_vec = np.ascontiguousarray(gens.g_vec, dtype=np.uint64), np.ascontiguousarray(gens.h_vec, dtype=np.uint64)
    if g_vec.shape != h_vec.shape or g_vec.shape[0] != N:
        raise ValueError(f"the generator vectors hold N = {N} points each")
    w = g_vec.shape[1]
    pb = 8 * w                                                    # bytes per point
    draw = drawer(rand, 2 * n_max + 12)
    s_l, s_r = draw(n_max), draw(n_max)
    bl_i, bl_o, bl_s, bl_w = draw(4)                        # aIBlinding, aOBlinding, sBlinding, gamma
    bufs = []
    clock = [time.perf_counter()]

    def lap(key):
        now = time.perf_counter()
        if stats is not None:
            stats[key] = stats.get(key, 0.0) + now - clock[0]
        clock[0] = now

    def up(arr):
        d = ctx.to_device(arr)
        bufs.append(d)
        return d

    def alloc(nbytes):
        d = ctx.dev_alloc(max(nbytes, 32))
        bufs.append(d)
        return d

    def up_csr(csr):
        row_ptr, col, coeff = csr
        col, coeff = np.asarray(col, dtype=np.uint32), np.asarray(coeff, dtype=np.uint64).reshape(-1, 4)
        if len(col) == 0:                                         # never read: any valid pointers
            col, coeff = np.zeros(1, dtype=np.uint32), np.zeros((1, 4), dtype=np.uint64)
        return up(np.asarray(row_ptr, dtype=np.uint32)), up(col), up(coeff)

    def point(jacs):
        return ctx.into_affine(c, 1, ctx.fold(c, 1, np.concatenate(jacs)))

    try:
        # ---- residency: generators, assignment, matrices, blinding vectors
        dg, dh = up(g_vec), up(h_vec)
        dgi, dhi = up(np.zeros(N, dtype=np.uint8)), up(np.zeros(N, dtype=np.uint8))
        d_gh = up(np.stack([np.asarray(gens.g, dtype=np.uint64).reshape(w), np.asarray(gens.h, dtype=np.uint64).reshape(w)]))
        d_h1, d_u = d_gh + pb, up(np.asarray(gens.u, dtype=np.uint64).reshape(w))
        d_f = up(fr_to_mont(f, c))
        d_w = d_f + 32 * k
        d_al, d_ar, d_ao, d_v = alloc(32 * n), alloc(32 * n), alloc(32 * n), alloc(32 * n_w)
        for which, out in (("a", d_al), ("b", d_ar), ("c", d_ao)):
            ctx.fr_spmv(c, *up_csr(r1cs.csr(which)), n, d_f, out)
        d_sl, d_sr = up(fr_to_mont(s_l, c)), up(fr_to_mont(s_r, c))
        lap("upload")
        # ---- A_I, A_O, A_W, S                                                          (:363-384)
        d_bl = up(fr_to_mont([bl_i, bl_o, bl_w, bl_s], c))
        jac = ctx.msm_var_batch_dev(
            c, 1, [dg, dh, d_h1, dg, d_h1, dg, d_h1, dg, dh, d_h1], [dgi, dhi, None, dgi, None, dgi, None, dgi, dhi, None],
            [d_al, d_ar, d_bl, d_ao, d_bl + 32, d_w, d_bl + 64, d_sl, d_sr, d_bl + 96], [n, n, 1, n, 1, n_w, 1, n_max, n_max, 1],
            montgomery=True)
        a_i, a_o, a_w, s_pt = point(jac[0:3]), point(jac[3:5]), point(jac[5:7]), point(jac[7:10])
        lap("commit_a")
        y, z = (int(t) % r for t in challenger.yz(a_i, a_o, a_w, s_pt))
        if y == 0:
            raise ValueError("the challenge y is zero")
        ym, zm = fr_mont(y, c), fr_mont(z, c)
        # ---- v = z_Q WV                                                                (:426-469)
        zn = pow(z, n, r)
        if n_w:
            d_zq, d_t = alloc(32 * n), [alloc(32 * n_w) for _ in range(3)]
            ctx.fr_powers_dev(c, zm, zm, d_zq, n)
            for which, out in zip("abc", d_t):
                ctx.fr_spmv(c, *up_csr(witness_transpose(r1cs.csr(which), k, n_w)), n_w, d_zq, out)
            ctx.fr_lincomb_dev(c, d_t, [n_w] * 3, fr_to_mont([1, zn, zn * zn % r], c), d_v, n_w)
        vecs = ctx.bp_vectors(d_al, d_ar, d_ao, d_w if n_w else 0, d_v if n_w else 0, d_sl, d_sr, n, n_w, n_max, N)
        lap("v")
        # ---- t(X) and T_i                                                              (:491-511)
        t = [fr_int(e, c) for e in ctx.fr_bp_t_coeffs_dev(c, vecs, ym, zm)]           # t_2 .. t_10
        taus = draw(8)
        d_ts = up(fr_to_mont([e for deg, tau in zip(T_DEGREES, taus) for e in (t[deg - 2], tau)], c))
        jac = ctx.msm_var_batch_dev(c, 1, [d_gh] * 8, None, [d_ts + 64 * i for i in range(8)], [2] * 8, montgomery=True)
        t_pts = [ctx.into_affine(c, 1, j) for j in jac]
        lap("t")
        x = int(challenger.x(list(t_pts))) % r
        # ---- l(x), r(x), t_x, tau_x, mu                                                 (:527-549)
        d_lx, d_rx = alloc(32 * N), alloc(32 * N)
        t_x = fr_int(ctx.fr_bp_lr_eval_dev(c, vecs, ym, zm, fr_mont(x, c), d_lx, d_rx), c)
        tau_x = sum(tau * pow(x, deg, r) for deg, tau in zip(T_DEGREES, taus)) % r
        mu = (bl_i * pow(x, 2, r) + bl_o * pow(x, 3, r) + bl_w * pow(x, 4, r) + bl_s * pow(x, 5, r)) % r
        l_x, r_x = np.zeros((N, 4), dtype=np.uint64), np.zeros((N, 4), dtype=np.uint64)
        ctx.d2h(l_x, d_lx)
        ctx.d2h(r_x, d_rx)
        lap("lr")
        x_1 = int(challenger.x1(t_x, tau_x, mu, l_x, r_x)) % r
        # ---- IPP_P = <l_x, g> + <r_x, h> + t_x (x_1 u)                                  (:561-566)
        d_c = up(fr_to_mont([x_1 * t_x, 0], c))
        jac = ctx.msm_var_batch_dev(c, 1, [dg, dh, d_u], [dgi, dhi, None], [d_lx, d_rx, d_c], [N, N, 1], montgomery=True)
        proof = Proof(a_i, a_o, a_w, s_pt, t_pts, mu, tau_x, l_x, r_x, t_x, point(jac))
        lap("ipp_p")
        # ---- the inner-product argument over a = l_x, b = r_x and x_1 u               (inner_product_proof.rs:46-102)
        length, cs = N, None
        while length > 1:
            m = length // 2
            al, ar, bl, br = d_lx, d_lx + 32 * m, d_rx, d_rx + 32 * m
            gl, gr, hl, hr = dg, dg + pb * m, dh, dh + pb * m
            if cs is None:                                        # later rounds: from the fold before
                cs = ctx.fr_dot_batch_dev(c, [al, ar], [br, bl], [m, m])
            ctx.h2d(d_c, fr_to_mont([x_1 * fr_int(cs[0], c), x_1 * fr_int(cs[1], c)], c))
            jac = ctx.msm_var_batch_dev(c, 1, [gr, hl, d_u, gl, hr, d_u], [dgi + m, dhi, None, dgi, dhi + m, None],
                                        [al, br, d_c, ar, bl, d_c + 32], [m, m, 1, m, m, 1], montgomery=True)
            l_pt, r_pt = point(jac[0:3]), point(jac[3:6])
            proof.L_vec.append(l_pt)
            proof.R_vec.append(r_pt)
            xr = int(challenger.ipa(l_pt, r_pt)) % r
            if xr == 0:
                raise ValueError("an inner-product challenge is zero")
            xm, xim = fr_mont(xr, c), fr_mont(pow(xr, -1, r), c)
            ctx.ipa_fold_dev(c, gl, dgi, gr, dgi + m, m, xim, xm, gl, dgi)       # g' = x^-1 gL + x gR
            ctx.ipa_fold_dev(c, hl, dhi, hr, dhi + m, m, xm, xim, hl, dhi)       # h' = x hL + x^-1 hR
            cs = ctx.fr_ipa_fold_ab_dev(c, d_lx, d_rx, length, xm)
            length = m
        ab = np.zeros((2, 4), dtype=np.uint64)
        ctx.d2h(ab[0], d_lx)
        ctx.d2h(ab[1], d_rx)
        proof.a, proof.b = fr_int(ab[0], c), fr_int(ab[1], c)
        lap("ipa")
        return proof
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
