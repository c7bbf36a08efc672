#!/usr/bin/env python3
"""Fused sum-check round (zkp_fr_sumcheck_round_dev, phase-one shape eq (a b - c)), the whole phase-one prover
(sumcheck.prove_phase_one) and the eq table (zkp_fr_eq_evals_dev).  HIP events around each call (zkp_timer_*), after warm-up; the
median of --reps (>= 20).  In the same process, for every size:
  * the UNFUSED composition of the same round from the exports that existed before the fused one (zkp_fr_vec_op_dev,
    zkp_fr_dot_batch_dev): bind every table (SUB, AXPY), step every table to the points 2 and 3 (SUB, ADD, ADD), a b - c per
    point (MUL, SUB) and one batched inner product against eq: 28 launches instead of 2;
  * the library's copy kernel (zkp_bench_hbm_copy) over the bytes the fused round moves (four tables read, their low halves
    written: 192 B per row of the tables): the memory floor of the round.
One JSON line per case.

    python tools/sumcheck_bench.py [--reps 20] [--quick]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import api, codec, sumcheck  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402

VEC_MUL, VEC_ADD, VEC_SUB, VEC_AXPY = 0, 1, 2, 4


def timed(ctx, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop_ms())
    return float(np.median(ts)), float(np.min(ts))


def rand_fr(rng, c, n):
    """n reduced values as Montgomery words (any words below r are a valid table for timing)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def unfused_round(ctx, c, tabs, n, x, tmp):
    """bind x into the four tables of n rows, then g(0), g(2), g(3) of eq (a b - c) over their bound halves"""
    m, h = n // 2, n // 4
    d, p, w, half = tmp[0:4], tmp[4:8], tmp[8:11], tmp[11]
    for t in tabs:                                                 # t[:m] += x (t[m:] - t[:m])
        ctx.fr_vec_op(c, VEC_SUB, t + 32 * m, t, half, m)
        ctx.fr_vec_op(c, VEC_AXPY, t, half, t, m, x)
    for i, t in enumerate(tabs):                                   # lo + 2 (hi - lo) = hi + d, lo + 3 (hi - lo) = hi + 2 d
        ctx.fr_vec_op(c, VEC_SUB, t + 32 * h, t, d[i], h)
        ctx.fr_vec_op(c, VEC_ADD, t + 32 * h, d[i], p[i], h)
    for k, src in enumerate((tabs, p)):
        ctx.fr_vec_op(c, VEC_MUL, src[1], src[2], w[k], h)
        ctx.fr_vec_op(c, VEC_SUB, w[k], src[3], w[k], h)
    eq2 = p[0]
    q = d                                                          # point 3 over the d buffers: q = p + d
    for i in range(4):
        ctx.fr_vec_op(c, VEC_ADD, p[i], d[i], q[i], h)
    ctx.fr_vec_op(c, VEC_MUL, q[1], q[2], w[2], h)
    ctx.fr_vec_op(c, VEC_SUB, w[2], q[3], w[2], h)
    return ctx.fr_dot_batch_dev(c, [tabs[0], eq2, q[0]], w, [h, h, h])


def case(ctx, curve, log_n, reps):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    host = rand_fr(rng, c, n)
    tabs = [ctx.dev_alloc(32 * n) for _ in range(4)]
    tmp = [ctx.dev_alloc(32 * (n // 4)) for _ in range(11)] + [ctx.dev_alloc(32 * (n // 2))]
    x = codec.fr_to_mont([0x1234567 + log_n], c)[0]
    out = []
    try:
        for i, t in enumerate(tabs):
            ctx.h2d(t, np.roll(host, 37 * i, axis=0))
        tag = {"curve": curve, "log_n": log_n}
        fused, fmin = timed(ctx, lambda: ctx.fr_sumcheck_round_dev(c, api.SC_EQ_AB_MINUS_C, tabs, n, bind=x), reps)
        first, _ = timed(ctx, lambda: ctx.fr_sumcheck_round_dev(c, api.SC_EQ_AB_MINUS_C, tabs, n), reps)
        unf, umin = timed(ctx, lambda: unfused_round(ctx, c, tabs, n, x, tmp), reps)
        moved = 192 * n
        gbs = ctx.bench_hbm_copy(max(moved // 2, 1 << 20))
        floor_ms = moved / (gbs * 1e9) * 1e3
        out.append(dict(tag, case="round_bind_eval", fused_ms=round(fused, 4), fused_min_ms=round(fmin, 4), unfused_ms=round(unf, 4),
                        unfused_min_ms=round(umin, 4), unfused_over_fused=round(unf / fused, 2), eval_only_ms=round(first, 4),
                        bytes_moved=moved, copy_gb_per_s=round(gbs, 1), copy_floor_ms=round(floor_ms, 4),
                        fused_over_floor=round(fused / floor_ms, 2),
                        floor_note="copy kernel: 1 read per write; the round: 2 reads per write, same total bytes"))
        if log_n <= 20:
            # the `par` shape of the cubic prover: 17 terms a_k b_k c that share c (35 tables), each term reduced in turn
            pool = ctx.dev_alloc(32 * (n + 37 * 35))
            try:
                ctx.h2d(pool, np.concatenate([host, host[:37 * 35]]))
                more = [ctx.dev_alloc(32 * n) for _ in range(31)]
                tmp_tabs = tabs + more
                for i, t in enumerate(more):
                    ctx.d2d(t, pool + 32 * 37 * (i + 1), 32 * n)
                par = [p for k in range(17) for p in (tmp_tabs[2 * k], tmp_tabs[2 * k + 1], tmp_tabs[34])]
                par_ms, _ = timed(ctx, lambda: ctx.fr_sumcheck_round_dev(c, api.SC_PROD3, par, n, bind=x), reps)
                out.append(dict(tag, case="round_bind_eval_par17", fused_ms=round(par_ms, 4), tables=35, bytes_moved=35 * 48 * n,
                                gb_per_s=round(35 * 48 * n / (par_ms * 1e-3) / 1e9, 1)))
            finally:
                ctx.sync()
                ctx.dev_free(pool)
                for t in more:
                    ctx.dev_free(t)

        def ch(coeffs):
            return int.from_bytes(hashlib.sha256(b"".join(v.to_bytes(32, "little") for v in coeffs)).digest(), "little") % c.r

        # the tables are bound in place, so every run sees other values: the time does not depend on them
        phase, _ = timed(ctx, lambda: sumcheck.prove_phase_one(ctx, c, *tabs, n, 0, ch), reps, warm=1)
        out.append(dict(tag, case="prove_phase_one", ms=round(phase, 3), rounds=log_n, calls=log_n + 1, ms_per_round=round(phase / log_n, 4)))
        rs = codec.fr_to_mont(list(range(3, 3 + log_n)), c)
        eqt, _ = timed(ctx, lambda: ctx.fr_eq_evals_dev(c, rs, tabs[0]), reps)
        out.append(dict(tag, case="eq_evals", ms=round(eqt, 4), gb_per_s_written=round(32 * n / (eqt * 1e-3) / 1e9, 1)))
    finally:
        ctx.sync()
        for p in tabs + tmp:
            ctx.dev_free(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="2^12 BN254, one whole phase only (for a kernel trace)")
    args = ap.parse_args()
    ctx = Context(0)
    cases = [("bn254", 12)] if args.quick else [("bn254", 16), ("bn254", 20), ("bn254", 24), ("bls12_381", 20)]
    for curve, log_n in cases:
        for line in case(ctx, curve, log_n, 1 if args.quick else max(args.reps, 20)):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
