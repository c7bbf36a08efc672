"""Hyrax's data-parallel GKR on the device: n copies of one layered circuit proved at once.  Circuit::evaluate per copy
(hyrax/src/circuit.rs:115-163), eval_outputs (evaluate.rs:11-50) and, per layer, the table work of ZkSumcheckProof::prover
(zk_sumcheck_proof.rs:83-442) in the loop of HyraxProof::prover (hyrax_proof.rs:92-147), every table resident on the device.

A layer over all copies is node-major: element i n + t is node i in copy t.  Per layer: w = u0 eq(ql) + u1 eq(qr) from the eq-table
and vector entry points; sum-check #1 over the copy variables is log2 n + 1 zkp_fr_gkr_dp_round_dev calls over a copy of the layer
below and eq(q') (the reference's per-gate table temp_vec[g][t] is w[g] eq[t]); the closing call leaves v = V(rs, .) for every
node.  Sum-checks #2 and #3 are Libra's two phases (gkr.py) with G := P = w eq[0]: phase one against w := v, phase two against
w := eq(r0) and fu := x, because eval_eq(convert_to_bit(i)) is the indicator vector of node i.

The Pedersen and packing commitments, the blinds, LogDotProductProof, EqProof and the merlin transcript are the caller's:
`next_round(coeffs)` receives a round polynomial ([d, c, b, a] or [c, b, a]) and returns the challenge, `next_u()` returns (u0, u1)
between layers.  Field elements are canonical Python integers; device tables are Montgomery Fr.  The wiring is gkr.Circuit."""
from __future__ import annotations

import time

import numpy as np

from . import gkr
from .api import VEC_AXPY, VEC_SCALE
from .codec import fr_int, fr_mont, fr_to_mont
from .params import get_curve
from .sumcheck import cubic_coeffs, evaluate_poly, first_element

HYRAX_THREADS = 256   # csrc/hyrax.hpp: columns (copies) per workgroup of the evaluation
HYRAX_CHUNK = 32      # entries of the by-left-node list per workgroup
LINCOMB_MAX = 32      # vectors per zkp_fr_lincomb_dev call


def _is_pow2(n: int) -> bool:
    return n >= 1 and n & (n - 1) == 0


def evaluate_batch(circuit: gkr.Circuit, curve, inputs, witnesses) -> list:
    """Circuit::evaluate for every copy: the DEVICE buffer of every layer, node-major, 2^bit_size rows of n = len(inputs) Montgomery
    Fr (the gates, then zero rows: hyrax_proof.rs:95-107).  The input layer of copy t is aux, zeros, inputs, zeros
    (circuit.rs:127-134), transposed on the host.  The caller frees them (gkr.free_evals)."""
    c = get_curve(curve)
    ctx = circuit.ctx
    n = len(inputs)
    if not _is_pow2(n) or len(witnesses) != n:
        raise ValueError("the number of copies is a power of two (hyrax_proof.rs:53)")
    half = 1 << (circuit.bit_sizes[0] - 1)
    cols = []
    for inp, aux in zip(inputs, witnesses):
        assert half >= len(inp) and half >= len(aux)
        cols.append(list(aux) + [0] * (half - len(inp)) + list(inp) + [0] * (half - len(aux)))
    values = [cols[t][i] % c.r for i in range(2 * half) for t in range(n)]
    evals = [ctx.to_device(fr_to_mont(values, c))]
    try:
        for d in range(1, circuit.depth):
            evals.append(ctx.dev_alloc((32 * n) << circuit.bit_sizes[d]))
            ctx.fr_gkr_eval_layer_batch_dev(c, circuit.handles[d], evals[d - 1], evals[d], n)
    except Exception:
        gkr.free_evals(circuit, evals)
        raise
    return evals


def read_layer(circuit: gkr.Circuit, curve, evals, d: int, n: int) -> list:
    """layer d as rows of integers: [node][copy], all 2^bit_size rows"""
    c = get_curve(curve)
    rows = 1 << circuit.bit_sizes[d]
    a = np.zeros((rows * n, 4), dtype=np.uint64)
    circuit.ctx.d2h(a, evals[d])
    flat = [fr_int(v, c) for v in a]
    return [flat[i * n:(i + 1) * n] for i in range(rows)]


def eval_outputs(circuit: gkr.Circuit, curve, evals, n: int, q, q_aside) -> int:
    """eval_outputs (evaluate.rs:11-50) at the points the caller drew: sum_t eq(q')[t] sum_g eq(q)[g] out[g][t].  The inner sums
    are linear combinations of the output rows, at most LINCOMB_MAX vectors per call; the outer one is one inner product."""
    c = get_curve(curve)
    ctx = circuit.ctx
    k = circuit.bit_sizes[-1]
    assert len(q) == k and 1 << len(q_aside) == n
    eq_q = ctx.fr_eq_evals(c, np.stack([fr_mont(t % c.r, c) for t in q]).reshape(-1, 4) if k else np.zeros((0, 4), np.uint64)).reshape(-1, 4)
    one = fr_mont(1, c)
    d_acc, d_eq = ctx.dev_alloc(32 * n), ctx.dev_alloc(32 * n)
    try:
        rows = [(evals[-1] + 32 * n * g, eq_q[g]) for g in range(circuit.counts[-1])]        # the zero rows add nothing
        first = True
        while rows:
            take = rows[:LINCOMB_MAX if first else LINCOMB_MAX - 1]
            rows = rows[len(take):]
            ptrs = [p for p, _ in take] + ([] if first else [d_acc])
            coeffs = [cf for _, cf in take] + ([] if first else [one])
            ctx.fr_lincomb_dev(c, ptrs, [n] * len(ptrs), np.stack(coeffs), d_acc, n)
            first = False
        gkr._eq_into(ctx, c, [t % c.r for t in q_aside], d_eq)
        return fr_int(ctx.fr_dot_batch_dev(c, [d_acc], [d_eq], [n])[0], c)
    finally:
        ctx.sync()
        ctx.dev_free(d_acc)
        ctx.dev_free(d_eq)


def eval_witness(ctx, curve, witnesses, q_aside, ql, qr) -> tuple:
    """eval_value(witness_vec, q' || ql[1:]) and (..., q' || qr[1:]) of hyrax_proof.rs:149-178: the copies' witnesses, each padded
    to a power of two, as one multilinear polynomial"""
    c = get_curve(curve)
    wl = 1 << gkr._log2_ceil(max(len(witnesses[0]), 1))
    if len(ql) < 1 or wl != 1 << (len(ql) - 1) or len(witnesses) != 1 << len(q_aside):
        raise ValueError("the padded witness fills the first half of the input layer")
    vec = [v for w in witnesses for v in list(w) + [0] * (wl - len(w))]
    d_w, d_eq = ctx.to_device(fr_to_mont(vec, c)), ctx.dev_alloc(32 * len(vec))
    try:
        out = []
        for tail in (ql, qr):
            gkr._eq_into(ctx, c, [t % c.r for t in list(q_aside) + list(tail[1:])], d_eq)
            out.append(fr_int(ctx.fr_dot_batch_dev(c, [d_w], [d_eq], [len(vec)])[0], c))
        return tuple(out)
    finally:
        ctx.dev_free(d_w)
        ctx.dev_free(d_eq)


def prove_layers(circuit: gkr.Circuit, curve, evals, n: int, q_aside, q, result_u, next_round, next_u, stats: dict | None = None):
    """The loop of HyraxProof::prover (hyrax_proof.rs:72-147) from the output points (q', q) and result_u = eval_outputs.
    Returns (proofs, q', ql, qr): proofs[i] = (polys, (rs, r0, r1), (x, y)) of layer depth - 1 - i, polys the log2 n cubics
    [d, c, b, a] of sum-check #1 (zk_sumcheck_proof.rs:160-177), then the quadratics [c, b, a] of #2 and of #3 (:290-300, :395-404);
    q', ql, qr the last layer's challenges, where the witness polynomial is opened.  stats (a dict) receives the host's wall
    seconds per part, summed over the layers: "weights", "sumcheck1", "sumcheck23" (every call returns when its work is done)."""
    c = get_curve(curve)
    r = c.r
    ctx = circuit.ctx
    assert _is_pow2(n) and 1 << len(q_aside) == n
    for d in range(1, circuit.depth):
        if circuit.counts[d] != 1 << circuit.bit_sizes[d]:
            raise ValueError("every layer needs a power-of-two gate count (zk_sumcheck_proof.rs:96)")
    log_n = n.bit_length() - 1
    rows_max = 1 << max(circuit.bit_sizes[:-1])
    g_max = 1 << max(circuit.bit_sizes[1:])
    bufs = [ctx.dev_alloc(32 * rows_max * n), ctx.dev_alloc(32 * n)] + [ctx.dev_alloc(32 * g_max) for _ in range(3)] + \
        [ctx.dev_alloc(32 * rows_max) for _ in range(5)]
    d_v, d_eq, d_w, d_t, d_g, d_fin, d_f, d_mul, d_a1, d_a2 = bufs
    u0, u1 = 1, 0
    q_aside = [t % r for t in q_aside]
    ql = [t % r for t in q]
    qr = list(ql)
    claim = result_u % r
    proofs = []
    try:
        for d in range(circuit.depth - 1, 0, -1):
            t0 = time.perf_counter()
            layer = circuit.handles[d]
            rows, g_len = 1 << circuit.bit_sizes[d - 1], 1 << circuit.bit_sizes[d]
            assert len(ql) == len(qr) == circuit.bit_sizes[d]
            # w = u0 eq(ql) + u1 eq(qr)                                              (xg_q, zk_sumcheck_proof.rs:84-88)
            gkr._eq_into(ctx, c, ql, d_w)
            ctx.fr_vec_op(c, VEC_SCALE, d_w, None, d_w, g_len, fr_mont(u0, c))
            if u1:
                gkr._eq_into(ctx, c, qr, d_t)
                ctx.fr_vec_op(c, VEC_AXPY, d_w, d_t, d_w, g_len, fr_mont(u1, c))
            gkr._eq_into(ctx, c, q_aside, d_eq)
            t1 = time.perf_counter()
            polys, rs = [], []
            if log_n:                                                                # sum-check #1 (:98-224)
                ctx.d2d(d_v, evals[d - 1], 32 * rows * n)
                length, x = n, None
                for _ in range(log_n):
                    ev = ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, length, bind=None if x is None else fr_mont(x, c))
                    if x is not None:
                        length //= 2
                    coeffs = cubic_coeffs(fr_int(ev[0], c), fr_int(ev[1], c), fr_int(ev[2], c), claim, r)
                    x = next_round(list(coeffs)) % r
                    claim = evaluate_poly(coeffs, x, r)
                    polys.append(coeffs)
                    rs.append(x)
                ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, length, bind=fr_mont(x, c), want_evals=False, finals_ptr=d_fin)
            else:
                ctx.d2d(d_fin, evals[d - 1], 32 * rows)
            t2 = time.perf_counter()
            # P = w eq[0]                                                            (temp_p_xg_vec, :225-227)
            ctx.fr_vec_op(c, VEC_SCALE, d_w, None, d_g, g_len, fr_mont(first_element(ctx, d_eq, c), c))
            # sum-check #2 = Libra's phase one with G := P, w := v                   (:241-346)
            ctx.fr_gkr_tables_dev(c, layer, 1, d_g, d_fin, [d_mul, d_a1, d_a2])
            ctx.d2d(d_f, d_fin, 32 * rows)
            polys_2, r0 = gkr._phase(ctx, c, 1, [d_f, d_mul, d_a1, d_a2], rows, claim, None, next_round)
            if polys_2:
                claim = evaluate_poly(polys_2[-1], r0[-1], r)
            x = first_element(ctx, d_f, c)
            # sum-check #3 = phase two with w := eq(r0), fu := x                     (:339-442)
            gkr._eq_into(ctx, c, r0, d_a2)
            ctx.fr_gkr_tables_dev(c, layer, 2, d_g, d_a2, [d_mul, d_a1])
            ctx.d2d(d_f, d_fin, 32 * rows)
            polys_3, r1 = gkr._phase(ctx, c, 2, [d_f, d_mul, d_a1], rows, claim, x, next_round)
            y = first_element(ctx, d_f, c)
            proofs.append((polys + polys_2 + polys_3, (rs, r0, r1), (x, y)))
            if stats is not None:
                for key, dt in (("weights", t1 - t0), ("sumcheck1", t2 - t1), ("sumcheck23", time.perf_counter() - t2)):
                    stats[key] = stats.get(key, 0.0) + dt
            q_aside, ql, qr = rs, r0, r1                                             # hyrax_proof.rs:125-127
            if d > 1:                                                                # :134-145
                u0, u1 = (v % r for v in next_u())
                claim = (x * u0 + y * u1) % r
        return proofs, q_aside, ql, qr
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
