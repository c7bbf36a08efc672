#!/usr/bin/env python3
"""PLONK evaluations and opening polynomials on the device: zkp_fr_poly_eval_many_dev, zkp_fr_lincomb_dev and rounds 4-5 of
ckb_zkp_amd.plonk.  HIP events around each call (zkp_timer_*), warm-up 3, the median of --reps (>= 20); the alternatives of a
comparison take turns inside one loop of one process and are checked to give identical words in the same run.  One JSON line per
case.  Each call is timed against
  (a) its composition from the exports that existed before it: 20 zkp_poly_evaluate_dev calls for the evaluation, one
      zkp_fr_vec_op_dev SCALE and 19 AXPY passes for the combination;
  (b) the library's copy kernel (zkp_bench_hbm_copy) over the bytes the call must move: 20 vectors read for the evaluation,
      20 read + 1 written for the combination;
  (c) rounds 4 and 5 (plonk.prover_fourth_round, plonk.prover_openings, everything left on the device) at 2^20 rows.

    python tools/plonk_open_bench.py [--reps 20] [--logs 12 14 ..] [--curves bn254 bls12_381] [--only a|c]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import codec, plonk  # noqa: E402
from ckb_zkp_amd.api import NTT_FFT, Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402

VEC_SCALE, VEC_AXPY = 3, 4
KS = [1, 7, 13, 17]
K = 20                                                             # the polynomials of rounds 4 and 5


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


def timed_host(ctx, fn, reps):
    """host clock around work that ends in a synchronise: (median, min) ms"""
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def rand_fr(rng, c, n):
    """n reduced values as Montgomery words (any words below r are a valid table for timing)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def floor_ms(ctx, moved):
    gbs = ctx.bench_hbm_copy(max(moved // 2, 1 << 20))
    return gbs, moved / (gbs * 1e9) * 1e3


def read(ctx, d, n):
    a = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(a, d)
    return a


def open_case(ctx, curve, log_n, reps):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(400 + log_n)
    host = rand_fr(rng, c, n)
    polys = [ctx.to_device(np.roll(host, 7 * k, axis=0)) for k in range(K)]
    out_a, out_b = ctx.dev_alloc(32 * n), ctx.dev_alloc(32 * n)
    z = rand_fr(rng, c, 1)[0]
    scalars = rand_fr(rng, c, K)
    ns = [n] * K
    res = {}
    try:
        def each():
            res["each"] = np.stack([ctx.poly_evaluate(c, p, n, z) for p in polys])

        def many():
            res["many"] = ctx.fr_poly_eval_many_dev(c, polys, ns, z)

        def chain():
            ctx.fr_vec_op(c, VEC_SCALE, polys[0], None, out_b, n, scalars[0])
            for k in range(1, K):
                ctx.fr_vec_op(c, VEC_AXPY, out_b, polys[k], out_b, n, scalars[k])

        te = timed_alternating(ctx, {"many": many, "each": each}, reps)
        tl = timed_alternating(ctx, {"fused": lambda: ctx.fr_lincomb_dev(c, polys, ns, scalars, out_a, n), "chain": chain}, reps)
        same_eval = bool(np.array_equal(res["many"], res["each"]))
        same_comb = bool(np.array_equal(read(ctx, out_a, n), read(ctx, out_b, n)))
        moved_e, moved_l = K * 32 * n, (K + 1) * 32 * n
        gbs_e, fl_e = floor_ms(ctx, moved_e)
        gbs_l, fl_l = floor_ms(ctx, moved_l)
        return [dict(case="eval_many", curve=curve, log_n=log_n, polys=K, many_ms=round(te["many"][0], 4), many_min_ms=round(te["many"][1], 4),
                     each_ms=round(te["each"][0], 4), each_min_ms=round(te["each"][1], 4), each_calls=K,
                     each_over_many=round(te["each"][0] / te["many"][0], 2), same_result=same_eval, bytes_moved=moved_e,
                     copy_gb_per_s=round(gbs_e, 1), copy_floor_ms=round(fl_e, 4), many_over_floor=round(te["many"][0] / fl_e, 2)),
                dict(case="lincomb", curve=curve, log_n=log_n, terms=K, fused_ms=round(tl["fused"][0], 4), fused_min_ms=round(tl["fused"][1], 4),
                     chain_ms=round(tl["chain"][0], 4), chain_min_ms=round(tl["chain"][1], 4), chain_launches=K,
                     chain_over_fused=round(tl["chain"][0] / tl["fused"][0], 2), same_result=same_comb, bytes_moved=moved_l,
                     chain_bytes_moved=(3 * K - 1) * 32 * n, copy_gb_per_s=round(gbs_l, 1), copy_floor_ms=round(fl_l, 4),
                     fused_over_floor=round(tl["fused"][0] / fl_l, 2))]
    finally:
        ctx.sync()
        for p in polys + [out_a, out_b]:
            ctx.dev_free(p)


def rounds_case(ctx, curve, log_n, reps):
    """rounds 4 and 5 after rounds 1-3 of a circuit whose copy constraints are the identity (sigma_j = ks_j w^i: every witness
    closes) with random selector and witness words: the time of a round does not depend on the values"""
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(500 + log_n)
    x = np.zeros((n, 4), dtype=np.uint64)
    x[1] = codec.fr_mont(1, c)
    roots, tmp = ctx.to_device(x), ctx.dev_alloc(32 * n)
    ctx.ntt_dev(c, roots, log_n, NTT_FFT)                              # w^i: the transform of the polynomial X
    sel = {"n": n}
    for j in range(4):
        ctx.fr_vec_op(c, VEC_SCALE, roots, None, tmp, n, codec.fr_mont(KS[j], c))
        sel[f"sigma_{j}"] = read(ctx, tmp, n)
    for p in (roots, tmp):
        ctx.dev_free(p)
    host = rand_fr(rng, c, n)
    for i, name in enumerate(plonk.SELECTORS[:7]):
        sel[name] = np.roll(host, 3 * i, axis=0)
    ix = plonk.Index(ctx, c, sel, KS, keep_coeffs=True)
    ps = plonk.prover_init(ix, np.roll(host, 101, axis=0))
    w = [np.roll(host, 17 * (j + 1), axis=0) for j in range(4)]
    zeta, eps = 0x123456789ABCDEF0123456789, 0xFEDCBA987654321
    try:
        plonk.prover_first_round(ps, w, to_host=False)
        plonk.prover_second_round(ps, 0x1234567, 0x7654321, to_host=False)
        plonk.prover_third_round(ps, 0xABCDEF01, to_host=False)
        r4 = lambda: plonk.prover_fourth_round(ps, zeta)                                   # noqa: E731
        r5 = lambda: plonk.prover_openings(ps, zeta, epsilon=eps, to_host=False)           # noqa: E731
        r4(), r5()                                                     # warm-up: scratch, code objects
        both = timed_host(ctx, lambda: (r4(), r5()), reps)
        t4, t5 = timed_host(ctx, r4, reps), timed_host(ctx, r5, reps)
        return [dict(case="rounds_4_5", curve=curve, log_n=log_n, ms=round(both[0], 2), min_ms=round(both[1], 2), reps=reps,
                     round4_ms=round(t4[0], 2), round5_ms=round(t5[0], 2),
                     note="host clock; round 4: 2 evaluation calls + host arithmetic; round 5: 1 combination + 2 divisions by X - z")]
    finally:
        ps.close()
        ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-whole", type=int, default=5)
    ap.add_argument("--only", choices=["a", "c"], default=None)
    ap.add_argument("--logs", type=int, nargs="*", default=None, help="log2 of the coefficients instead of 12, 14, .., 22")
    ap.add_argument("--curves", nargs="*", default=["bn254"], help="BLS12-381 runs the same kernels with its own multiplier")
    args = ap.parse_args()
    ctx = Context(0)
    reps = max(args.reps, 20)
    emit = lambda lines: [print(json.dumps(line), flush=True) for line in lines]    # noqa: E731
    if args.only in (None, "a"):
        for curve in args.curves:
            for log_n in args.logs or (12, 14, 16, 18, 20, 22):
                emit(open_case(ctx, curve, log_n, reps))
    if args.only in (None, "c"):
        for curve in args.curves:
            emit(rounds_case(ctx, curve, 20, args.reps_whole))


if __name__ == "__main__":
    main()
