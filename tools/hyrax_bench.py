#!/usr/bin/env python3
"""Hyrax's data-parallel GKR on the device: the sum-check over the copies (zkp_fr_gkr_dp_round_dev), the batched layer evaluation
(zkp_fr_gkr_eval_layer_batch_dev) and a whole hyrax.prove_layers.  HIP events around each alternative (zkp_timer_*), warm-up 3, the
median of --reps (>= 20); the alternatives of a comparison take turns inside one loop of one process; both are checked to give
the same words in the same run.  One JSON line per case.  A layer has G gates over 2 G nodes (uniform wiring), n copies.
  (a) round 0 and a whole sum-check #1 (log2 n + 1 calls) through zkp_fr_gkr_dp_round_dev, against the composition from the
      exports that existed before it: the G x n tables temp[g] = w[g] eq built with zkp_fr_vec_op_dev (one time, reported apart),
      then per round zkp_fr_sumcheck_round_dev with one ZKP_SC_PROD3 term (temp[g], V[left], V[right]) per mul gate and two
      (temp[g], V[left], 1), (temp[g], V[right], 1) per add gate, at most 256 terms per call, evaluations added on the host; the
      bind of a round is bind-only calls over every distinct table once.
  (b) the library's copy kernel (zkp_bench_hbm_copy) over the bytes the fused calls must move: every live element of V and eq read
      once per evaluation, read and written once per bind.
  (c) zkp_fr_gkr_eval_layer_batch_dev against n calls of zkp_fr_gkr_eval_layer_dev on a copy-major table (at most 1024 calls are
      timed and scaled to n).
  (d) hyrax.prove_layers per layer, split into sum-check #1 and #2 + #3 (host wall time, driver included).

    python tools/hyrax_bench.py [--reps 20] [--quick] [--only a|c|d]
--quick: one call of every kind at a small shape and nothing else (for a kernel trace that counts launches).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import codec, gkr, hyrax  # noqa: E402
from ckb_zkp_amd.api import SC_PROD3, VEC_SCALE, Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402

MAX_TERMS = 256


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


def wiring(rng, n_gates, nodes):
    return (rng.integers(0, 2, size=n_gates, dtype=np.uint8), rng.integers(0, nodes, size=n_gates, dtype=np.uint32),
            rng.integers(0, nodes, size=n_gates, dtype=np.uint32))


class Composed:
    """sum-check #1 from zkp_fr_vec_op_dev + zkp_fr_sumcheck_round_dev: its own copy of V, the G x n temp tables, a table of ones"""

    def __init__(self, ctx, c, op, left, right, nodes, n, d_v_src, d_eq, w_host):
        self.ctx, self.c, self.n, self.nodes, self.g = ctx, c, n, nodes, len(op)
        self.d_v_src = d_v_src
        self.d_v = ctx.dev_alloc(32 * nodes * n)
        self.d_temp = ctx.dev_alloc(32 * self.g * n)
        self.d_ones = ctx.to_device(np.tile(codec.fr_mont(1, c), (n, 1)))
        self.d_eq, self.w_host = d_eq, w_host
        row = lambda i: self.d_v + 32 * n * int(i)                # noqa: E731
        terms = []
        for g in range(self.g):
            t = self.d_temp + 32 * n * g
            terms += [(t, row(left[g]), row(right[g]))] if op[g] else [(t, row(left[g]), self.d_ones), (t, row(right[g]), self.d_ones)]
        self.calls = [[p for term in terms[i:i + MAX_TERMS] for p in term] for i in range(0, len(terms), MAX_TERMS)]
        distinct = [self.d_temp + 32 * n * g for g in range(self.g)] + [row(i) for i in range(nodes)] + [self.d_ones]
        self.bind_calls = []
        for i in range(0, len(distinct), 3 * MAX_TERMS):
            part = distinct[i:i + 3 * MAX_TERMS]
            part += [part[-1]] * (-len(part) % 3)                  # a table named twice in one call is bound once
            self.bind_calls.append(part)
        self.reset()

    def reset(self):
        """fresh V and temp[g] = w[g] eq (the one-time build)"""
        ctx, c, n = self.ctx, self.c, self.n
        ctx.d2d(self.d_v, self.d_v_src, 32 * self.nodes * n)
        ctx.h2d(self.d_ones, np.tile(codec.fr_mont(1, c), (n, 1)))
        for g in range(self.g):
            ctx.fr_vec_op(c, VEC_SCALE, self.d_eq, None, self.d_temp + 32 * n * g, n, self.w_host[g])

    def evaluate(self, length):
        c, r = self.c, self.c.r
        tot = [0, 0, 0]
        for tabs in self.calls:
            ev = self.ctx.fr_sumcheck_round_dev(c, SC_PROD3, tabs, length)
            for term in ev:
                for p in range(3):
                    tot[p] += codec.fr_int(term[p], c)
        return tuple(t % r for t in tot)

    def evaluate_untallied(self, length):
        """the device work and the read-backs alone: what the timing compares"""
        for tabs in self.calls:
            self.ctx.fr_sumcheck_round_dev(self.c, SC_PROD3, tabs, length)

    def bind(self, length, x):
        for part in self.bind_calls:
            self.ctx.fr_sumcheck_round_dev(self.c, SC_PROD3, part, length, bind=x, want_evals=False)

    def whole(self, x):
        length = self.n
        self.evaluate_untallied(length)
        while length > 2:
            self.bind(length, x)
            length //= 2
            self.evaluate_untallied(length)
        self.bind(length, x)

    def free(self):
        for p in (self.d_v, self.d_temp, self.d_ones):
            self.ctx.dev_free(p)


def fused_whole(ctx, c, layer, d_v, d_eq, d_w, d_fin, n, x):
    length = n
    ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, length)
    while length > 2:
        ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, length, bind=x)
        length //= 2
    ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, length, bind=x, want_evals=False, finals_ptr=d_fin)


def sumcheck_case(ctx, curve, log_g, log_n, reps, compose=True):
    c = get_curve(curve)
    g, nodes, n = 1 << log_g, 2 << log_g, 1 << log_n
    rng = np.random.default_rng(100 * log_g + log_n)
    op, left, right = wiring(rng, g, nodes)
    layer = ctx.gkr_layer_upload(op, left, right, log_g + 1)
    v_host = rand_fr(rng, c, nodes * n)
    d_src, d_v = ctx.to_device(v_host), ctx.dev_alloc(32 * nodes * n)
    del v_host
    eq_host, w_host = rand_fr(rng, c, n), rand_fr(rng, c, g)
    d_eq_src, d_eq, d_w, d_fin = ctx.to_device(eq_host), ctx.dev_alloc(32 * n), ctx.to_device(w_host), ctx.dev_alloc(32 * nodes)
    x = codec.fr_mont(0x1234567 + log_n, c)
    comp = None
    ints = lambda ev: tuple(codec.fr_from_mont(ev, c))            # noqa: E731
    try:
        info = ctx.gkr_layer_info(layer)
        ctx.d2d(d_v, d_src, 32 * nodes * n)
        ctx.d2d(d_eq, d_eq_src, 32 * n)
        line = dict(case="sumcheck1", curve=curve, log_gates=log_g, log_copies=log_n, max_fan_left=info["max_fan_left"])
        same = None
        if compose:
            ctx.timer_start()
            comp = Composed(ctx, c, op, left, right, nodes, n, d_src, d_eq_src, w_host)
            line["temp_build_ms"] = round(ctx.timer_stop_ms(), 3)
            # the same words: round 0, then one bound round (each side binds its own tables)
            same = ints(ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, n)) == comp.evaluate(n)
            if n >= 4:
                got = ints(ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, n, bind=x))
                comp.bind(n, x)
                same = same and got == comp.evaluate(n // 2)
            line["composed_calls_round0"] = len(comp.calls)
        fns = {"fused_round0": lambda: ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, n),
               "fused_whole": lambda: fused_whole(ctx, c, layer, d_v, d_eq, d_w, d_fin, n, x)}
        if compose:
            fns["composed_round0"] = lambda: comp.evaluate_untallied(n)
            fns["composed_whole"] = lambda: comp.whole(x)
        t = timed_alternating(ctx, fns, reps)                      # the tables keep being bound in place: the time does not depend on the values
        elems_eval0 = (nodes + 1) * n                              # (b): every live element once per evaluation, read + written per bind
        elems_whole = elems_eval0 + sum((nodes + 1) * (ln + ln // 2 + (ln // 2 if ln > 2 else 0)) for ln in [n >> i for i in range(log_n)])
        gbs = ctx.bench_hbm_copy(max(16 * elems_eval0, 1 << 20))
        floor0, floor_w = 32 * elems_eval0 / (gbs * 1e9) * 1e3, 32 * elems_whole / (gbs * 1e9) * 1e3
        for k, (med, mn) in t.items():
            line[k + "_ms"], line[k + "_min_ms"] = round(med, 4), round(mn, 4)
        line.update(same_evals=same, copy_gb_per_s=round(gbs, 1), copy_floor_round0_ms=round(floor0, 4), copy_floor_whole_ms=round(floor_w, 4),
                    fused_round0_over_floor=round(t["fused_round0"][0] / floor0, 2), fused_whole_over_floor=round(t["fused_whole"][0] / floor_w, 2))
        if compose:
            line.update(composed_over_fused_round0=round(t["composed_round0"][0] / t["fused_round0"][0], 2),
                        composed_over_fused_whole=round(t["composed_whole"][0] / t["fused_whole"][0], 2))
        return [line]
    finally:
        ctx.sync()
        if comp:
            comp.free()
        for p in (d_src, d_v, d_eq_src, d_eq, d_w, d_fin):
            ctx.dev_free(p)
        ctx.gkr_layer_free(layer)


def eval_case(ctx, curve, log_g, log_n, reps):
    c = get_curve(curve)
    g, nodes, n = 1 << log_g, 2 << log_g, 1 << log_n
    rng = np.random.default_rng(7 + 100 * log_g + log_n)
    op, left, right = wiring(rng, g, nodes)
    layer = ctx.gkr_layer_upload(op, left, right, log_g + 1)
    host = rand_fr(rng, c, nodes * n)                              # copy-major: [copy][node]
    d_cm = ctx.to_device(host)
    d_nm = ctx.to_device(np.ascontiguousarray(host.reshape(n, nodes, 4).transpose(1, 0, 2)).reshape(-1, 4))
    d_out_cm, d_out_nm = ctx.dev_alloc(32 * g * n), ctx.dev_alloc(32 * g * n)
    calls = min(n, 1024)
    try:
        def per_copy(count):
            for t in range(count):
                ctx.fr_gkr_eval_layer_dev(c, layer, d_cm + 32 * nodes * t, d_out_cm + 32 * g * t)

        per_copy(n)
        ctx.fr_gkr_eval_layer_batch_dev(c, layer, d_nm, d_out_nm, n)
        a, b = np.zeros((g * n, 4), np.uint64), np.zeros((g * n, 4), np.uint64)
        ctx.d2h(a, d_out_cm)
        ctx.d2h(b, d_out_nm)
        same = bool(np.array_equal(a.reshape(n, g, 4).transpose(1, 0, 2), b.reshape(g, n, 4)))
        t = timed_alternating(ctx, {"batch": lambda: ctx.fr_gkr_eval_layer_batch_dev(c, layer, d_nm, d_out_nm, n), "per_copy": lambda: per_copy(calls)}, reps)
        per_copy_ms = t["per_copy"][0] * n / calls
        return [dict(case="eval_layer", curve=curve, log_gates=log_g, log_copies=log_n, batch_ms=round(t["batch"][0], 4),
                     batch_min_ms=round(t["batch"][1], 4), per_copy_calls_timed=calls, per_copy_ms=round(per_copy_ms, 3),
                     scaled=calls != n, per_copy_over_batch=round(per_copy_ms / t["batch"][0], 1), same_values=same)]
    finally:
        ctx.sync()
        for p in (d_cm, d_nm, d_out_cm, d_out_nm):
            ctx.dev_free(p)
        ctx.gkr_layer_free(layer)


def _challenges(c):
    def h(*parts):
        return int.from_bytes(hashlib.sha256(b"".join(int(v).to_bytes(32, "little") for v in parts)).digest(), "little") % c.r
    return (lambda coeffs: h(*coeffs)), (lambda: (h(1), h(2)))


def whole_case(ctx, curve, layers, log_g, log_n, reps):
    c = get_curve(curve)
    g, n = 1 << log_g, 1 << log_n
    rng = np.random.default_rng(9)
    raw = [np.stack([a.astype(np.int64) for a in wiring(rng, g, 2 * g if i == 0 else g)], axis=1) for i in range(layers)]
    circuit = gkr.Circuit(ctx, g, g, raw)
    evals = [ctx.to_device(rand_fr(rng, c, 2 * g * n))]           # the input layer, node-major, straight from random words
    try:
        for d in range(1, circuit.depth):
            evals.append(ctx.dev_alloc((32 * n) << circuit.bit_sizes[d]))
            ctx.fr_gkr_eval_layer_batch_dev(c, circuit.handles[d], evals[d - 1], evals[d], n)
        vals = codec.limbs_to_ints(rand_fr(rng, c, log_g + log_n))
        q, qa = vals[:log_g], vals[log_g:]
        result_u = hyrax.eval_outputs(circuit, c, evals, n, q, qa)
        runs = []
        for _ in range(reps + 1):
            stats = {}
            ctx.timer_start()
            hyrax.prove_layers(circuit, c, evals, n, qa, q, result_u, *_challenges(c), stats=stats)
            stats["total_ms"] = ctx.timer_stop_ms()
            runs.append(stats)
        runs = runs[1:]                                            # the first run is the warm-up
        med = lambda k: float(np.median([s[k] for s in runs]))    # noqa: E731
        return [dict(case="prove_layers", curve=curve, layers=layers, log_gates=log_g, log_copies=log_n, reps=reps,
                     total_ms=round(med("total_ms"), 2), per_layer_ms=round(med("total_ms") / layers, 2),
                     sumcheck1_ms_per_layer=round(1e3 * med("sumcheck1") / layers, 2),
                     sumcheck23_ms_per_layer=round(1e3 * med("sumcheck23") / layers, 2),
                     weights_ms_per_layer=round(1e3 * med("weights") / layers, 2),
                     calls_per_layer=dict(sumcheck1=log_n + 1, sumcheck23=2 * (log_g + 1) + 2),
                     note="host wall time per part (every call returns when its work is done), host driver included")]
    finally:
        gkr.free_evals(circuit, evals)
        circuit.free()


def quick(ctx):
    """one call of every kind, no warm-up, so that a kernel trace shows the launches per call"""
    c = get_curve("bn254")
    log_g, n = 8, 1 << 10
    g, nodes = 1 << log_g, 2 << log_g
    rng = np.random.default_rng(1)
    layer = ctx.gkr_layer_upload(*wiring(rng, g, nodes), log_g + 1)
    d_v, d_eq, d_w = ctx.to_device(rand_fr(rng, c, nodes * n)), ctx.to_device(rand_fr(rng, c, n)), ctx.to_device(rand_fr(rng, c, g))
    d_out, d_fin = ctx.dev_alloc(32 * g * n), ctx.dev_alloc(32 * nodes)
    x = codec.fr_mont(77, c)
    ctx.fr_gkr_eval_layer_batch_dev(c, layer, d_v, d_out, n)
    ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, n)
    ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, n, bind=x)
    ctx.fr_gkr_dp_round_dev(c, layer, d_v, d_eq, d_w, n, 2, bind=x, want_evals=False, finals_ptr=d_fin)
    ctx.sync()
    for p in (d_v, d_eq, d_w, d_out, d_fin):
        ctx.dev_free(p)
    ctx.gkr_layer_free(layer)
    print(json.dumps(dict(case="quick", shape=dict(log_gates=log_g, log_copies=10),
                          calls=["eval_layer_batch: 1 launch", "round 0, evaluate: 2 launches", "bind + evaluate: 3 launches",
                                 "closing call, bind + finals: 1 launch"],
                          expected_kernel_calls=dict(hyrax_eval_kernel=1, hyrax_round_kernel=2, fr_sum_partials_kernel=2, hyrax_bind_kernel=2))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-whole", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one call of every kind at 2^8 gates x 2^10 copies (for a kernel trace)")
    ap.add_argument("--only", choices=["a", "c", "d"], default=None)
    ap.add_argument("--log-gates", type=int, nargs="*", default=None)
    ap.add_argument("--log-total", type=int, nargs="*", default=None, help="log2 (gates x copies)")
    args = ap.parse_args()
    ctx = Context(0)
    if args.quick:
        return quick(ctx)
    reps = max(args.reps, 20)
    emit = lambda lines: [print(json.dumps(line), flush=True) for line in lines]    # noqa: E731
    shapes = [(lg, lt - lg) for lg in args.log_gates or (6, 10, 14) for lt in args.log_total or (16, 20, 24)]
    if args.only in (None, "a"):
        for lg, ln in shapes:
            emit(sumcheck_case(ctx, "bn254", lg, ln, reps))
        for lg, ln in ((10, 10), (14, 10)):
            emit(sumcheck_case(ctx, "bls12_381", lg, ln, reps))
    if args.only in (None, "c"):
        for lg, ln in shapes:
            emit(eval_case(ctx, "bn254", lg, ln, reps))
        emit(eval_case(ctx, "bls12_381", 10, 10, reps))
    if args.only in (None, "d"):
        emit(whole_case(ctx, "bn254", 4, 10, 10, args.reps_whole))
        emit(whole_case(ctx, "bls12_381", 4, 10, 10, args.reps_whole))


if __name__ == "__main__":
    main()
