"""Libra's linear-time GKR on the device: Circuit::new / Circuit::evaluate (libra/src/circuit.rs:116-185), eval_output
(evaluate.rs:11-33) and the layer loop of LinearGKRProof::prover (libra_linear_gkr.rs:51-110), every table resident on the device.

Per layer: G = alpha eq(gu) + beta eq(gv) from the eq-table and vector entry points, ONE zkp_fr_gkr_tables_dev call for the three
tables of eval_hg, phase one over a copy of V, then eq(ru), ONE tables call for eval_fgu and phase two.  A phase of v rounds is
v + 1 zkp_fr_gkr_round_dev calls, as in sumcheck.py: the last one only binds and leaves the final values at element 0.

The reference's transcript (and, in the ZK variant, its commitments and blinds) is the caller's: `next_round(coeffs)` receives a
round polynomial [c, b, a] and returns the challenge, `absorb_final(values)` sees a phase's final values, `next_alpha_beta()`
returns (alpha, beta) between layers.  Field elements are canonical Python integers; device tables are Montgomery Fr."""
from __future__ import annotations

import numpy as np

from .api import VEC_AXPY, VEC_SCALE
from .codec import fr_int, fr_mont, fr_to_mont
from .params import get_curve
from .sumcheck import evaluate_poly, first_element, quadratic_coeffs

GKR_LONG = 256        # csrc/gkr.hpp: a node with more gates than this is summed by workgroups, not by one thread
GKR_CHUNK = 4096      # entries per workgroup of such a node


def _log2_ceil(n: int) -> int:
    return (n - 1).bit_length()


class Circuit:
    """Circuit::new: the input layer of Layer::input_new (circuit.rs:40-53) and one wiring handle per layer of layers_raw
    (lists of (op, left, right), op 0 = add / 1 = mul).  counts[d] / bit_sizes[d]: gates_count / bit_size of layer d."""

    def __init__(self, ctx, num_inputs: int, num_aux: int, layers_raw):
        self.ctx = ctx
        gates = 1 << _log2_ceil(max(num_aux, num_inputs, 1))
        self.counts, self.bit_sizes, self.handles = [2 * gates], [_log2_ceil(2 * gates)], [None]
        try:
            for raw in layers_raw:
                if not len(raw):
                    raise ValueError("a layer without gates")
                a = np.asarray(raw, dtype=np.int64).reshape(-1, 3)
                if a[:, 0].min() < 0 or a[:, 0].max() > 1:
                    raise ValueError("IllegalOperator")                          # circuit.rs:61-63
                if a[:, 1:].min() < 0 or a[:, 1:].max() >= self.counts[-1]:
                    raise ValueError("IllegalNode")                              # circuit.rs:64-66
                self.handles.append(ctx.gkr_layer_upload(a[:, 0], a[:, 1], a[:, 2], self.bit_sizes[-1]))
                self.counts.append(len(a))
                self.bit_sizes.append(_log2_ceil(len(a)))
        except Exception:
            self.free()
            raise
        self.depth = len(self.counts)

    def info(self, d: int) -> dict:
        return self.ctx.gkr_layer_info(self.handles[d])

    def free(self):
        for h in self.handles:
            if h:
                self.ctx.gkr_layer_free(h)
        self.handles = [None] * len(self.handles)


def evaluate(circuit: Circuit, curve, inputs, aux) -> list:
    """Circuit::evaluate: the DEVICE buffer of every layer, 2^bit_size Montgomery Fr each (the gates, then zeros).  The input layer
    is assembled on the host as circuit.rs:149-156 does: aux, zeros, inputs, zeros.  The caller frees them (free_evals)."""
    c = get_curve(curve)
    ctx = circuit.ctx
    half = 1 << (circuit.bit_sizes[0] - 1)
    assert half >= len(inputs) and half >= len(aux)
    values = list(aux) + [0] * (half - len(inputs)) + list(inputs) + [0] * (half - len(aux))
    evals = [ctx.to_device(fr_to_mont(values, c))]
    try:
        for d in range(1, circuit.depth):
            evals.append(ctx.dev_alloc(32 << circuit.bit_sizes[d]))
            ctx.fr_gkr_eval_layer_dev(c, circuit.handles[d], evals[d - 1], evals[d])
    except Exception:
        free_evals(circuit, evals)
        raise
    return evals


def free_evals(circuit: Circuit, evals):
    for p in evals:
        circuit.ctx.dev_free(p)


def read_layer(circuit: Circuit, curve, evals, d: int) -> list:
    """the gates_count values of layer d as integers"""
    c = get_curve(curve)
    a = np.zeros((circuit.counts[d], 4), dtype=np.uint64)
    circuit.ctx.d2h(a, evals[d])
    return [fr_int(v, c) for v in a]


def _eq_into(ctx, c, rs, d_out):
    ctx.fr_eq_evals_dev(c, np.stack([fr_mont(t, c) for t in rs]).reshape(-1, 4) if len(rs) else np.zeros((0, 4), np.uint64), d_out)


def eval_output(circuit: Circuit, curve, evals, gu) -> int:
    """eval_output (evaluate.rs:11-33) at the point gu the caller drew: eval_value of the zero-padded output layer"""
    c = get_curve(curve)
    ctx = circuit.ctx
    k = circuit.bit_sizes[-1]
    assert len(gu) == k
    d_eq = ctx.dev_alloc(32 << k)
    try:
        _eq_into(ctx, c, gu, d_eq)
        return fr_int(ctx.fr_dot_batch_dev(c, [evals[-1]], [d_eq], [1 << k])[0], c)
    finally:
        ctx.dev_free(d_eq)


def _phase(ctx, c, phase, tables, n, claim, fu, next_round):
    """phase_one_prover / phase_two_prover (sumcheck.rs:42-87, 118-162) over DEVICE tables: (polys, challenges)"""
    r = c.r
    polys, rs = [], []
    length, x = n, None
    fu_m = None if fu is None else fr_mont(fu, c)
    for _ in range(n.bit_length() - 1):
        ev = ctx.fr_gkr_round_dev(c, phase, tables, length, fu=fu_m, bind=None if x is None else fr_mont(x, c))
        if x is not None:
            length //= 2
        coeffs = quadratic_coeffs(fr_int(ev[0], c), fr_int(ev[1], c), claim, r)
        x = next_round(list(coeffs)) % r
        claim = evaluate_poly(coeffs, x, r)
        polys.append(coeffs)
        rs.append(x)
    if x is not None:
        ctx.fr_gkr_round_dev(c, phase, tables, length, fu=fu_m, bind=fr_mont(x, c), want_evals=False)
    return polys, rs


def prove_layers(circuit: Circuit, curve, evals, gu, result_u, next_round, absorb_final, next_alpha_beta):
    """The loop of LinearGKRProof::prover (libra_linear_gkr.rs:38-110) from the output point gu and result_u = eval_output.
    Returns (proofs, ru, rv): proofs[i] = (polys_1, finals_1, polys_2, finals_2) of layer depth - 1 - i with
    finals_1 = [f, mul, add1, add2] and finals_2 = [f, mul, add] (poly_value_at_r), ru / rv the last layer's challenges."""
    c = get_curve(curve)
    r = c.r
    ctx = circuit.ctx
    for d in range(circuit.depth - 1):
        if circuit.counts[d] != 1 << circuit.bit_sizes[d]:
            raise ValueError("a layer that feeds another needs a power-of-two gate count (sumcheck.rs:32-35)")
    n_max = 1 << max(circuit.bit_sizes[:-1])
    g_max = 1 << max(circuit.bit_sizes[1:])
    bufs = [ctx.dev_alloc(32 * n_max) for _ in range(4)] + [ctx.dev_alloc(32 * g_max) for _ in range(2)]
    d_f, d_mul, d_a1, d_a2, d_g, d_t = bufs
    alpha, beta = 1, 0
    gu = [x % r for x in gu]
    gv = [0] * len(gu)
    result_u, result_v = result_u % r, 0
    proofs, ru, rv = [], [], []
    try:
        for d in range(circuit.depth - 1, 0, -1):
            claim = (alpha * result_u + beta * result_v) % r
            n, g_len = 1 << circuit.bit_sizes[d - 1], 1 << circuit.bit_sizes[d]
            layer, d_v = circuit.handles[d], evals[d - 1]
            # G = alpha eq(gu) + beta eq(gv)                                         (initialize_phase_one, :210-215)
            _eq_into(ctx, c, gu, d_g)
            ctx.fr_vec_op(c, VEC_SCALE, d_g, None, d_g, g_len, fr_mont(alpha, c))
            if beta:
                _eq_into(ctx, c, gv, d_t)
                ctx.fr_vec_op(c, VEC_AXPY, d_g, d_t, d_g, g_len, fr_mont(beta, c))
            # phase one: f = V, (mul, add1, add2) = eval_hg                          (:55-72)
            ctx.fr_gkr_tables_dev(c, layer, 1, d_g, d_v, [d_mul, d_a1, d_a2])
            ctx.d2d(d_f, d_v, 32 * n)
            polys_1, ru = _phase(ctx, c, 1, [d_f, d_mul, d_a1, d_a2], n, claim, None, next_round)
            finals_1 = [first_element(ctx, p, c) for p in (d_f, d_mul, d_a1, d_a2)]
            absorb_final(list(finals_1))
            claim = (finals_1[0] * finals_1[1] + finals_1[0] * finals_1[2] + finals_1[3]) % r
            fu = finals_1[0]                                                       # V(ru): eval_ru of initialize_phase_two (:236)
            # phase two: f = V, (mul, add) = eval_fgu against eq(ru)                 (:74-91)
            _eq_into(ctx, c, ru, d_a2)
            ctx.fr_gkr_tables_dev(c, layer, 2, d_g, d_a2, [d_mul, d_a1])
            ctx.d2d(d_f, d_v, 32 * n)
            polys_2, rv = _phase(ctx, c, 2, [d_f, d_mul, d_a1], n, claim, fu, next_round)
            finals_2 = [first_element(ctx, p, c) for p in (d_f, d_mul, d_a1)]
            absorb_final(list(finals_2))
            proofs.append((polys_1, finals_1, polys_2, finals_2))
            if d > 1:                                                              # :98-109
                gu, gv = list(ru), list(rv)
                result_u, result_v = fu, finals_2[0]
                alpha, beta = (v % r for v in next_alpha_beta())
        return proofs, ru, rv
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
