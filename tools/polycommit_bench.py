#!/usr/bin/env python3
"""zkp_pedersen_commit_rows_dev against its composition from the exports that existed before it: one zkp_msm_g1_var_batch_dev call
over aliased bases (entry i: row i over the generators; entry rows + i: blind_i h), then one zkp_g1_fold and one zkp_g1_into_affine
per row on the host.  HIP events around each alternative (zkp_timer_*), every window ends in a synchronise; after a warm-up the
alternatives take turns inside one loop of one process, the composition twice per turn (composed / composed_again: the spread
between two runs of the same work), medians of --reps.  `batch_ms` times the batch call alone, so the share of the per-row host
calls is visible.  Both are checked to give the same words at every timed size.  One JSON line per (curve, rows, cols):
  * gadds_per_s: rows cols W bucket additions / time, against zkp_bench_mulmod's sustained Fq rate (unsaturated limbs) of the same
    run divided by the 13.5 product-equivalents of one XYZZ addition;
  * verdict: "faster" / "slower" only when the difference exceeds the composition's own spread, else "within spread".
Then zkp_fr_vecmat_dev at the same shapes: the bytes it must read (the matrix once) over its time against zkp_bench_hbm_copy, and
its rows cols products against zkp_bench_mulmod's Fr rate — whichever fraction is larger bounds it.  Then key creation at
n_gens = 2^10 and 2^16, and the wall time per stage of polycommit.reduce_prover at --open-vars (each stage ends in a synchronise).

    python tools/polycommit_bench.py [--reps 5] [--logs 5 8 10 12] [--open-vars 20] [--curves bn254 bls12_381] [--only-commit LOG]
--only-commit LOG runs zkp_pedersen_commit_rows_dev alone at 2^LOG x 2^LOG (for a kernel trace).
Runs on the GPU only: creating the context fails without one."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import codec, polycommit as pc  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402

ADD_PRODUCTS = 13.5                       # product-equivalents of one XYZZ addition (bucket_dev.hpp)


def rand_fr(rng, c, n):
    """n reduced values as Montgomery words (any words below r are a valid vector)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def gens(ctx, c, n, seed):
    rng = random.Random(seed)
    base = codec.g1_to_mont([c.g1], c)[0][0]
    return ctx.fixed_base_mul(c, 1, base, codec.fr_canonical([rng.randrange(1, c.r) for _ in range(n)], c))


def timed(ctx, fns, reps):
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ctx.timer_start()
            fn()
            ts[name].append(ctx.timer_stop_ms())
    return {name: float(np.median(v)) for name, v in ts.items()}


def commit_case(ctx, c, key, d_gens, d_h, log, reps, ceiling_adds, info):
    rows = cols = 1 << log
    w = 2 * c.fq_limbs
    rng = np.random.default_rng(log)
    d_s, d_b = ctx.to_device(rand_fr(rng, c, rows * cols)), ctx.to_device(rand_fr(rng, c, rows))
    xy, inf = np.zeros((rows, w), dtype=np.uint64), np.zeros(rows, dtype=np.uint8)
    d_xy, d_inf = ctx.to_device(xy), ctx.to_device(inf)
    try:
        def fused():
            ctx.pedersen_commit_rows_dev(key, d_s, rows, cols, d_b, d_xy, d_inf)
            ctx.sync()

        def batch():
            return ctx.msm_var_batch_dev(c, 1, [d_gens] * rows + [d_h] * rows, None, [d_s + 32 * cols * i for i in range(rows)] +
                                         [d_b + 32 * i for i in range(rows)], [cols] * rows + [1] * rows, montgomery=True)

        def composed():
            jac = batch()
            return [ctx.into_affine(c, 1, ctx.fold(c, 1, np.concatenate([jac[i], jac[rows + i]]))) for i in range(rows)]

        fused()
        ctx.d2h(xy, d_xy)
        ctx.d2h(inf, d_inf)
        want = composed()
        same = all(np.array_equal(xy[i], want[i][0]) and bool(inf[i]) == want[i][1] for i in range(rows))
        med = timed(ctx, {"fused": fused, "composed": composed, "composed_again": composed, "batch": batch}, reps)
    finally:
        for p in (d_s, d_b, d_xy, d_inf):
            ctx.dev_free(p)
    spread = abs(med["composed"] - med["composed_again"])
    comp = min(med["composed"], med["composed_again"])
    verdict = "within spread" if abs(med["fused"] - comp) <= spread else ("faster" if med["fused"] < comp else "slower")
    adds = rows * cols * info["W"] / (med["fused"] * 1e-3) / 1e9
    return dict(case="commit_rows", curve=c.name, rows=rows, cols=cols, same_words=bool(same), reps=reps,
                launches=dict(fused=info["launches"], composed="2 + 2 host calls per row"), fused_ms=round(med["fused"], 4),
                composed_ms=round(med["composed"], 4), composed_again_ms=round(med["composed_again"], 4), batch_ms=round(med["batch"], 4),
                spread_ms=round(spread, 4), composed_over_fused=round(comp / med["fused"], 2),
                batch_over_fused=round(med["batch"] / med["fused"], 2), verdict=verdict, gadds_per_s=round(adds, 3),
                mulmod_ceiling_gadds_per_s=round(ceiling_adds, 3), of_ceiling=round(adds / ceiling_adds, 3))


def vecmat_case(ctx, c, log, reps, hbm, fr_rate):
    rows = cols = 1 << log
    rng = np.random.default_rng(100 + log)
    d_l, d_m, d_o = ctx.to_device(rand_fr(rng, c, rows)), ctx.to_device(rand_fr(rng, c, rows * cols)), ctx.dev_alloc(32 * cols)
    try:
        def run():
            ctx.fr_vecmat_dev(c, d_l, d_m, rows, cols, d_o)
            ctx.sync()
        run()
        ms = timed(ctx, {"vecmat": run}, reps)["vecmat"]
    finally:
        for p in (d_l, d_m, d_o):
            ctx.dev_free(p)
    gbs = 32 * rows * cols / (ms * 1e-3) / 1e9
    gprod = rows * cols / (ms * 1e-3) / 1e9
    return dict(case="vecmat", curve=c.name, rows=rows, cols=cols, reps=reps, ms=round(ms, 4), bytes_read=32 * rows * cols,
                gbytes_per_s=round(gbs, 1), hbm_copy_gbytes_per_s=round(hbm, 1), of_hbm_copy=round(gbs / hbm, 3),
                gproducts_per_s=round(gprod, 2), mulmod_ceiling_gproducts_per_s=round(fr_rate, 1), of_mulmod=round(gprod / fr_rate, 4),
                bound_by="memory" if gbs / hbm >= gprod / fr_rate else "multiplier")


def key_case(ctx, c, xy, inf, h, n):
    t0 = time.perf_counter()
    key = ctx.pedersen_key_create(c, xy[:n], inf[:n], h)
    ms = 1e3 * (time.perf_counter() - t0)
    info = ctx.pedersen_key_info(key)
    ctx.pedersen_key_free(key)
    return dict(case="key_create", curve=c.name, n_gens=n, ms=round(ms, 2), table_mib=round(info["table_bytes"] / 2**20, 1),
                note="host wall time of the call: staging, 2 W launches, synchronise")


def open_case(ctx, c, s, reps):
    P = pc.setup(ctx, c, s, "open bench")
    rng = np.random.default_rng(s)
    pyr = random.Random(s)
    n = 1 << s
    l_size, r_size = pc.split_sizes(s)
    poly = pc.DevicePoly(ctx, c, rand_fr(rng, c, n))
    ry = [pyr.randrange(c.r) for _ in range(s)]

    class Challenger:                     # any function of the transcript: the timing does not depend on it
        def append(self, label, point):
            pass

        def challenge(self, label):
            return pyr.randrange(1, c.r)
    runs = []
    try:
        for _ in range(reps + 1):
            stats = {}
            t0 = time.perf_counter()
            comms, blinds = pc.packing_poly_commit(P, poly, lambda: pyr.randrange(c.r), True)
            stats["ms_commit"] = 1e3 * (time.perf_counter() - t0)
            pc.reduce_prover(P, poly, blinds, ry, pyr.randrange(c.r), pyr.randrange(c.r), lambda: pyr.randrange(c.r), Challenger(), stats)
            runs.append(stats)
    finally:
        poly.free()
        P.free()
    runs = runs[1:]                       # the first run is the warm-up
    return dict(case="reduce_prover", curve=c.name, num_vars=s, rows=l_size, cols=r_size, reps=reps,
                **{k: round(float(np.median([r[k] for r in runs])), 3) for k in runs[0]},
                note="host wall time per stage; ms_commit is packing_poly_commit (blinds' conversion and read-back included), "
                     "the eval claim is arbitrary: the prover's work does not depend on it")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logs", type=int, nargs="*", default=[5, 8, 10, 12])
    ap.add_argument("--open-vars", type=int, default=20)
    ap.add_argument("--curves", nargs="*", default=["bn254", "bls12_381"])
    ap.add_argument("--only-commit", type=int, default=0)
    args = ap.parse_args()
    ctx = Context(0)                                               # no GPU: this raises
    reps = max(args.reps, 3)
    hbm = ctx.bench_hbm_copy() if not args.only_commit else 0.0
    for name in args.curves:
        c = get_curve(name)
        logs = [args.only_commit] if args.only_commit else args.logs
        n_max = 1 << max(logs + [10])
        xy, inf = gens(ctx, c, (1 << 16) + 1 if not args.only_commit else n_max + 1, "bench " + name)
        h = xy[-1]
        key = ctx.pedersen_key_create(c, xy[:n_max], inf[:n_max], h)
        info = ctx.pedersen_key_info(key)
        d_gens, d_h = ctx.to_device(xy[:n_max]), ctx.to_device(h)
        try:
            if args.only_commit:
                rows = 1 << args.only_commit
                rng = np.random.default_rng(1)
                d_s, d_b = ctx.to_device(rand_fr(rng, c, rows * rows)), ctx.to_device(rand_fr(rng, c, rows))
                d_xy, d_inf = ctx.dev_alloc(16 * c.fq_limbs * rows), ctx.dev_alloc(rows)
                for _ in range(3):
                    ctx.pedersen_commit_rows_dev(key, d_s, rows, rows, d_b, d_xy, d_inf)
                    ctx.fr_vecmat_dev(c, d_b, d_s, rows, rows, d_xy)
                ctx.sync()
                for p in (d_s, d_b, d_xy, d_inf):
                    ctx.dev_free(p)
                continue
            ceiling = ctx.bench_mulmod(c, 1, True) / ADD_PRODUCTS
            fr_rate = ctx.bench_mulmod(c, 0, False)
            print(json.dumps(dict(case="key_info", curve=c.name, **{k: int(v) for k, v in info.items()})), flush=True)
            for log in logs:
                print(json.dumps(commit_case(ctx, c, key, d_gens, d_h, log, reps, ceiling, info)), flush=True)
            for log in logs:
                print(json.dumps(vecmat_case(ctx, c, log, reps, hbm, fr_rate)), flush=True)
            for n in (1 << 10, 1 << 16):
                print(json.dumps(key_case(ctx, c, xy, inf, h, n)), flush=True)
        finally:
            ctx.sync()
            ctx.pedersen_key_free(key)
            ctx.dev_free(d_gens)
            ctx.dev_free(d_h)
        if args.open_vars and not args.only_commit:
            print(json.dumps(open_case(ctx, c, args.open_vars, reps)), flush=True)


if __name__ == "__main__":
    main()
