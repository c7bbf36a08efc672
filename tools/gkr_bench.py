#!/usr/bin/env python3
"""Libra GKR on the device: the bookkeeping tables (zkp_fr_gkr_tables_dev), the fused round (zkp_fr_gkr_round_dev) and a whole
gkr.prove_layers.  HIP events around each call (zkp_timer_*), after warm-up; the median of --reps (>= 20); the alternatives of a
comparison take turns inside one loop of one process.  One JSON line per case.
  (a) tables: the one-pass call against its composition from the exports that existed before it: zkp_fr_gather_dev of G per
      entry of the node-grouped gate list (a coefficient array), then one zkp_fr_spmv_dev per table (phase 1: mul and add2
      against V, add1 against a vector of ones; phase 2: mul and add against eq(ru)).  2^16, 2^20, 2^24 gates over as many nodes,
      uniform wiring and wiring where one node feeds 40 % of the gates on both wires.
  (b) round: bind + evaluate in one pass against the same round from zkp_fr_vec_op_dev + zkp_fr_dot_batch_dev (bind: SUB, AXPY per
      table; point 2: SUB, ADD per table; sums: one batched inner product, against a vector of ones where a table is summed
      alone), and the library's copy kernel (zkp_bench_hbm_copy) over the bytes the fused round moves (48 B per row per table).
  (c) gkr.prove_layers over 8 layers of 2^20 gates (median of --reps-whole).

    python tools/gkr_bench.py [--reps 20] [--quick] [--only a|b|c]
--quick: 2^12, every kind of call exactly once and nothing else (for a kernel trace that counts launches).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import codec, gkr  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402

VEC_MUL, VEC_ADD, VEC_SUB, VEC_AXPY = 0, 1, 2, 4


def timed_alternating(ctx, fns, reps, warm=3):
    """{name: (median, min)} with the alternatives taking turns"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ctx.timer_start()
            fn()
            ts[k].append(ctx.timer_stop_ms())
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ts.items()}


def rand_fr(rng, c, n):
    """n reduced values as Montgomery words (any words below r are a valid table for timing)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def wiring(rng, n_gates, nodes, hot_share):
    op = rng.integers(0, 2, size=n_gates, dtype=np.uint8)
    left = rng.integers(0, nodes, size=n_gates, dtype=np.uint32)
    right = rng.integers(0, nodes, size=n_gates, dtype=np.uint32)
    if hot_share:
        left[rng.random(n_gates) < hot_share] = 5
        right[rng.random(n_gates) < hot_share] = 5
    return op, left, right


class Composition:
    """the node-grouped lists one side of a layer needs when the tables are built from zkp_fr_gather_dev + zkp_fr_spmv_dev:
    mul entries then add entries, each sorted by node (stable: gate order within a node)"""

    def __init__(self, ctx, op, key, other, nodes):
        self.ctx, self.nodes, self.n = ctx, nodes, len(op)
        parts = []
        for kind in (1, 0):
            g = np.flatnonzero(op == kind)
            g = g[np.argsort(key[g], kind="stable")]
            ptr = np.zeros(nodes + 1, dtype=np.uint32)
            ptr[1:] = np.cumsum(np.bincount(key[g], minlength=nodes))
            parts.append((g, ptr))
        self.n_mul = len(parts[0][0])
        order = np.concatenate([parts[0][0], parts[1][0]])
        self.bufs = [ctx.to_device(a) for a in (order.astype(np.int32), other[order].astype(np.uint32), np.zeros(self.n, dtype=np.uint32),
                                                parts[0][1], parts[1][1])]
        self.bufs.append(ctx.dev_alloc(32 * max(self.n, 1)))
        self.idx, self.col, self.col0, self.ptr_mul, self.ptr_add, self.coeff = self.bufs

    def run(self, c, phase, d_g, d_w, d_ones, outs):
        ctx, nm = self.ctx, self.n_mul
        ctx.fr_gather(d_g, self.idx, self.n, self.coeff)
        ctx.fr_spmv(c, self.ptr_mul, self.col, self.coeff, self.nodes, d_w, outs[0])
        if phase == 1:
            ctx.fr_spmv(c, self.ptr_add, self.col0 + 4 * nm, self.coeff + 32 * nm, self.nodes, d_ones, outs[1])
            ctx.fr_spmv(c, self.ptr_add, self.col + 4 * nm, self.coeff + 32 * nm, self.nodes, d_w, outs[2])
        else:
            ctx.fr_spmv(c, self.ptr_add, self.col + 4 * nm, self.coeff + 32 * nm, self.nodes, d_w, outs[1])

    def free(self):
        for p in self.bufs:
            self.ctx.dev_free(p)


def ones(ctx, c, n):
    return ctx.to_device(np.tile(codec.fr_mont(1, c), (n, 1)))


def tables_case(ctx, curve, log_n, hot_share, reps, check=True):
    c = get_curve(curve)
    n = nodes = 1 << log_n
    rng = np.random.default_rng(log_n + (1000 if hot_share else 0))
    op, left, right = wiring(rng, n, nodes, hot_share)
    layer = ctx.gkr_layer_upload(op, left, right, log_n)
    comps = [Composition(ctx, op, left, right, nodes), Composition(ctx, op, right, left, nodes)]
    host = rand_fr(rng, c, n)
    d_g, d_w, d_ones = ctx.to_device(host), ctx.to_device(np.roll(host, 41, axis=0)), ones(ctx, c, nodes)
    outs = [ctx.dev_alloc(32 * nodes) for _ in range(6)]
    lines = []
    try:
        info = ctx.gkr_layer_info(layer)
        for phase in (1, 2):
            k = 4 - phase
            new, old = outs[:k], outs[3:3 + k]
            fns = {"one_pass": lambda: ctx.fr_gkr_tables_dev(c, layer, phase, d_g, d_w, new),
                   "composed": lambda: comps[phase - 1].run(c, phase, d_g, d_w, d_ones, old)}
            t = timed_alternating(ctx, fns, reps)
            same = None
            if check:                                              # both ways give the same tables
                a, b = np.zeros((nodes, 4), np.uint64), np.zeros((nodes, 4), np.uint64)
                same = True
                for p, q in zip(new, old):
                    ctx.d2h(a, p)
                    ctx.d2h(b, q)
                    same = same and bool(np.array_equal(a, b))
            lines.append(dict(case="tables", curve=curve, log_gates=log_n, wiring="hot40" if hot_share else "uniform", phase=phase,
                              long_segments=info["long_left" if phase == 1 else "long_right"],
                              max_fan=info["max_fan_left" if phase == 1 else "max_fan_right"],
                              one_pass_ms=round(t["one_pass"][0], 4), one_pass_min_ms=round(t["one_pass"][1], 4),
                              composed_ms=round(t["composed"][0], 4), composed_min_ms=round(t["composed"][1], 4),
                              composed_over_one_pass=round(t["composed"][0] / t["one_pass"][0], 2), same_tables=same))
    finally:
        ctx.sync()
        for p in outs + [d_g, d_w, d_ones]:
            ctx.dev_free(p)
        for cp in comps:
            cp.free()
        ctx.gkr_layer_free(layer)
    return lines


def composed_round(ctx, c, phase, tabs, n, x, fu_int, tmp, d_ones):
    """bind x into the tables of n rows, then g(0), g(2) over their bound halves from vector ops and batched inner products"""
    m, h = n // 2, n // 4
    nt = len(tabs)
    d, p2, s, half = tmp[0:4], tmp[4:8], tmp[8:10], tmp[10]
    for t in tabs:                                                 # t[:m] += x (t[m:] - t[:m])
        ctx.fr_vec_op(c, VEC_SUB, t + 32 * m, t, half, m)
        ctx.fr_vec_op(c, VEC_AXPY, t, half, t, m, x)
    for i, t in enumerate(tabs):                                   # lo + 2 (hi - lo) = hi + (hi - lo)
        ctx.fr_vec_op(c, VEC_SUB, t + 32 * h, t, d[i], h)
        ctx.fr_vec_op(c, VEC_ADD, t + 32 * h, d[i], p2[i], h)
    r = c.r
    if phase == 1:                                                 # f (mul + add1) + add2
        ctx.fr_vec_op(c, VEC_ADD, tabs[1], tabs[2], s[0], h)
        ctx.fr_vec_op(c, VEC_ADD, p2[1], p2[2], s[1], h)
        v = [codec.fr_int(e, c) for e in ctx.fr_dot_batch_dev(c, [tabs[0], tabs[3], p2[0], p2[3]], [s[0], d_ones, s[1], d_ones], [h] * 4)]
        return (v[0] + v[1]) % r, (v[2] + v[3]) % r
    assert nt == 3                                                 # fu (mul f + add) + add f
    v = [codec.fr_int(e, c) for e in ctx.fr_dot_batch_dev(c, [tabs[1], tabs[2], tabs[2], p2[1], p2[2], p2[2]],
                                                          [tabs[0], d_ones, tabs[0], p2[0], d_ones, p2[0]], [h] * 6)]
    return (fu_int * (v[0] + v[1]) + v[2]) % r, (fu_int * (v[3] + v[4]) + v[5]) % r


def round_case(ctx, curve, log_n, reps):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    host = rand_fr(rng, c, n)
    tabs = [ctx.dev_alloc(32 * n) for _ in range(4)]
    tmp = [ctx.dev_alloc(32 * (n // 4)) for _ in range(10)] + [ctx.dev_alloc(32 * (n // 2))]
    d_ones = ones(ctx, c, n // 4)
    x = codec.fr_mont(0x1234567 + log_n, c)
    fu_int = 0x7654321
    fu = codec.fr_mont(fu_int, c)
    lines = []
    try:
        for phase in (1, 2):
            tb = tabs[:5 - phase]

            def reset():
                for i, t in enumerate(tb):
                    ctx.h2d(t, np.roll(host, 37 * i, axis=0))

            # the same values from both (each binds the tables in place, so each starts from fresh tables)
            reset()
            got = tuple(codec.fr_from_mont(ctx.fr_gkr_round_dev(c, phase, tb, n, fu=fu, bind=x), c))
            reset()
            same = got == composed_round(ctx, c, phase, tb, n, x, fu_int, tmp, d_ones)
            # timing: the tables keep being bound in place; the time does not depend on the values
            t = timed_alternating(ctx, {"fused": lambda: ctx.fr_gkr_round_dev(c, phase, tb, n, fu=fu, bind=x),
                                        "composed": lambda: composed_round(ctx, c, phase, tb, n, x, fu_int, tmp, d_ones),
                                        "eval_only": lambda: ctx.fr_gkr_round_dev(c, phase, tb, n, fu=fu)}, reps)
            moved = 48 * len(tb) * n
            gbs = ctx.bench_hbm_copy(max(moved // 2, 1 << 20))
            floor_ms = moved / (gbs * 1e9) * 1e3
            lines.append(dict(case="round_bind_eval", curve=curve, log_len=log_n, phase=phase, fused_ms=round(t["fused"][0], 4),
                              fused_min_ms=round(t["fused"][1], 4), composed_ms=round(t["composed"][0], 4),
                              composed_min_ms=round(t["composed"][1], 4), composed_over_fused=round(t["composed"][0] / t["fused"][0], 2),
                              eval_only_ms=round(t["eval_only"][0], 4), same_evals=bool(same), bytes_moved=moved,
                              copy_gb_per_s=round(gbs, 1), copy_floor_ms=round(floor_ms, 4), fused_over_floor=round(t["fused"][0] / floor_ms, 2)))
    finally:
        ctx.sync()
        for p in tabs + tmp + [d_ones]:
            ctx.dev_free(p)
    return lines


def _challenges(c):
    def h(*parts):
        return int.from_bytes(hashlib.sha256(b"".join(int(v).to_bytes(32, "little") for v in parts)).digest(), "little") % c.r
    return (lambda coeffs: h(*coeffs)), (lambda values: None), (lambda: (h(1), h(2)))


def whole_case(ctx, curve, layers, log_n, reps):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(7)
    raw = [np.stack([a.astype(np.int64) for a in wiring(rng, n, n, 0)], axis=1) for _ in range(layers)]
    vals = codec.limbs_to_ints(rand_fr(rng, c, n))
    circuit = gkr.Circuit(ctx, n // 2, n // 2, raw)
    evals = None
    try:
        ctx.timer_start()
        evals = gkr.evaluate(circuit, c, vals[:n // 2], vals[n // 2:])
        eval_ms = ctx.timer_stop_ms()
        gu = vals[:log_n]
        result_u = gkr.eval_output(circuit, c, evals, gu)
        ts = []
        for i in range(reps + 1):
            ctx.timer_start()
            gkr.prove_layers(circuit, c, evals, gu, result_u, *_challenges(c))
            ts.append(ctx.timer_stop_ms())
        ts = ts[1:]                                                # the first run is the warm-up
        return [dict(case="prove_layers", curve=curve, layers=layers, log_gates=log_n, ms=round(float(np.median(ts)), 2),
                     min_ms=round(float(np.min(ts)), 2), reps=reps, evaluate_ms=round(eval_ms, 2),
                     calls_per_layer=2 * (log_n + 1) + 2, note="wall of the device queue between HIP events, host driver included")]
    finally:
        if evals is not None:
            gkr.free_evals(circuit, evals)
        circuit.free()


def quick(ctx):
    """2^12: one call of every kind, no warm-up, so that a kernel trace shows the launches per call"""
    c = get_curve("bn254")
    log_n = 12
    n = 1 << log_n
    rng = np.random.default_rng(1)
    host = rand_fr(rng, c, n)
    d = [ctx.to_device(np.roll(host, 3 * i, axis=0)) for i in range(6)]
    x = codec.fr_mont(77, c)
    plan = []
    for share in (0, 0.4):
        layer = ctx.gkr_layer_upload(*wiring(rng, n, n, share), log_n)
        info = ctx.gkr_layer_info(layer)
        if not share:
            ctx.fr_gkr_eval_layer_dev(c, layer, d[0], d[2])
            plan.append("eval_layer: 1 launch")
        ctx.fr_gkr_tables_dev(c, layer, 1, d[0], d[1], d[2:5])
        plan.append(f"tables phase 1, {info['long_left']} long segments: {3 if info['long_left'] else 1} launches")
        ctx.gkr_layer_free(layer)
    ctx.fr_gkr_round_dev(c, 1, d[1:5], n)
    ctx.fr_gkr_round_dev(c, 2, d[1:4], n, fu=x, bind=x)
    ctx.fr_gkr_round_dev(c, 1, d[1:5], n, bind=x, want_evals=False)
    plan += ["round phase 1, evaluate: 2 launches", "round phase 2, bind + evaluate: 2 launches", "round phase 1, bind only: 1 launch"]
    ctx.sync()
    for p in d:
        ctx.dev_free(p)
    print(json.dumps(dict(case="quick", calls=plan, expected_kernel_calls=dict(gkr_eval_kernel=1, gkr_tables_kernel=2, gkr_chunk_kernel=1,
                                                                              gkr_long_kernel=1, gkr_round_kernel=2, gkr_final_kernel=2,
                                                                              gkr_bind_kernel=1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-whole", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="2^12 BN254, one call of every kind (for a kernel trace)")
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--logs", type=int, nargs="*", default=None, help="sizes of (a) / (b) instead of the defaults")
    args = ap.parse_args()
    ctx = Context(0)
    if args.quick:
        return quick(ctx)
    reps = max(args.reps, 20)
    emit = lambda lines: [print(json.dumps(line), flush=True) for line in lines]    # noqa: E731
    if args.only in (None, "a"):
        for log_n in args.logs or (16, 20, 24):
            for share in (0, 0.4):
                emit(tables_case(ctx, "bn254", log_n, share, reps))
        emit(tables_case(ctx, "bls12_381", 20, 0.4, reps))
    if args.only in (None, "b"):
        for log_n in args.logs or (12, 16, 20, 24):
            emit(round_case(ctx, "bn254", log_n, reps))
        emit(round_case(ctx, "bls12_381", 20, reps))
    if args.only in (None, "c"):
        emit(whole_case(ctx, "bn254", 8, 20, args.reps_whole))


if __name__ == "__main__":
    main()
