#!/usr/bin/env python3
"""zkp_g1_ntt_dev and asvc.prove_all against what the exports before them could do.  One JSON line per case, per curve:

  * g1_ntt: the forward transform in place at --logs (HIP events around the call, zkp_timer_*, median of --reps after one warm-up;
    the buffer keeps being transformed, the work per call is the same), with the scalar multiplications it performs,
    (n / 2) (log_n - 1), and the time per stage;
  * g1_ntt_composed at --compose-logs: the same transform as n MSMs of n points in ONE zkp_msm_g1_var_batch_dev call over a
    Vandermonde matrix of scalars that lies ready on the device (its n zkp_fr_powers_dev calls are not timed), results read back as
    Jacobian points as that entry does; three outputs are made affine and compared with zkp_g1_ntt_dev's words.  O(n^2) point work:
    the sizes stop where the matrix would take 2 GB.  `crossover` names the first measured size at which the transform wins;
  * prove_all at --prove-logs: host wall time of asvc.prove_all (it ends in a synchronise; median of --reps after one warm-up) with
    its per-stage split, the one-time all_proofs_key, and asvc.prove_pos(pk, values, [i]) at 64 seeded positions after one warm-up:
    n x its median is what all n proofs cost without the transform.  The 64 proofs are compared word for word with prove_all's;
  * copy_floor: the bytes of the buffers prove_all touches (A, the scalars, the 2n work points and flags), once read and once
    written, and per butterfly stage, over zkp_bench_hbm_copy's measured rate: the time below which no arrangement of this data
    flow can go.

    python tools/asvc_all_bench.py [--reps 5] [--logs 10 13 16] [--compose-logs 6 7 8 9 10] [--prove-logs 12 16]
                                   [--curves bn254 bls12_381] [--out profiles/asvc_all_bench.txt]
Runs on the GPU only: creating the context fails without one."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import asvc, codec  # noqa: E402
from ckb_zkp_amd.api import NTT_FFT, Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402

TAU = 0x1234567890ABCDEF1234567890ABCDEF


def rand_fr(rng, c, n):
    """n reduced values as words (any words below r are a valid vector)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def rand_points(ctx, c, rng, n):
    gen_xy, _ = codec.g1_to_mont([c.g1], c)
    return ctx.fixed_base_mul(c, 1, gen_xy[0], rand_fr(rng, c, n))


def timed(ctx, fn, reps):
    fn()                                                           # warm-up
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop_ms())
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def ntt_case(ctx, c, log_n, reps):
    n = 1 << log_n
    xy, inf = rand_points(ctx, c, np.random.default_rng(log_n), n)
    d_xy, d_inf = ctx.to_device(xy), ctx.to_device(inf)
    try:
        med, lo, hi = timed(ctx, lambda: ctx.g1_ntt_dev(c, d_xy, d_inf, log_n, NTT_FFT), reps)
    finally:
        ctx.sync()
        ctx.dev_free(d_xy)
        ctx.dev_free(d_inf)
    muls = (n // 2) * (log_n - 1)
    return dict(case="g1_ntt", curve=c.name, log_n=log_n, reps=reps, ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3),
                launches=log_n + 2, scalar_multiplications=muls, ms_per_stage=round(med / log_n, 3),
                us_per_scalar_multiplication=round(1e3 * med / max(muls, 1), 3))


def composed_case(ctx, c, log_n, reps):
    n = 1 << log_n
    xy, inf = rand_points(ctx, c, np.random.default_rng(100 + log_n), n)
    w = asvc.domain_root(c, n)
    d_xy, d_rows = ctx.to_device(xy), ctx.dev_alloc(32 * n * n)
    bufs = [d_xy, d_rows]
    try:
        one = codec.fr_mont(1, c)
        for i in range(n):                                         # row i: w^(i j), j < n
            ctx.fr_powers_dev(c, one, codec.fr_mont(pow(w, i, c.r), c), d_rows + 32 * n * i, n)
        ctx.sync()
        rows = [d_rows + 32 * n * i for i in range(n)]
        out = {}

        def run():
            out["jac"] = ctx.msm_var_batch_dev(c, 1, [d_xy] * n, None, rows, [n] * n, montgomery=True)

        med, lo, hi = timed(ctx, run, reps)
        d_t, d_ti = ctx.to_device(xy), ctx.to_device(inf)
        bufs += [d_t, d_ti]
        ntt_med, _, _ = timed(ctx, lambda: ctx.g1_ntt_dev(c, d_t, d_ti, log_n, NTT_FFT), reps)
        got_xy, got_inf = ctx.g1_ntt(c, xy, inf, NTT_FFT)
        same = all(np.array_equal(ctx.into_affine(c, 1, out["jac"][i])[0], got_xy[i]) and not got_inf[i] for i in (0, 1, n - 1))
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
    return dict(case="g1_ntt_composed", curve=c.name, log_n=log_n, reps=reps, same_words=bool(same), composed_ms=round(med, 3),
                composed_min_ms=round(lo, 3), composed_max_ms=round(hi, 3), g1_ntt_ms=round(ntt_med, 3),
                composed_over_g1_ntt=round(med / ntt_med, 2), msm_terms=n * n)


def prove_case(ctx, c, log_n, reps):
    n = 1 << log_n
    rng = np.random.default_rng(200 + log_n)
    gen_xy, _ = codec.g1_to_mont([c.g1], c)
    p1, _ = ctx.fixed_base_mul(c, 1, gen_xy[0], codec.fr_canonical([pow(TAU, j, c.r) for j in range(n + 1)], c))
    pk = asvc.ProvingKey(c, n, p1, p1[:n], p1[:n], p1[:n]).upload(ctx)    # prove_pos and prove_all read powers_of_g1 only
    values = codec.fr_from_mont(rand_fr(rng, c, n), c)
    positions = sorted({0, n // 2, n - 1} | {int(p) for p in rng.choice(n, size=61, replace=False)})[:64]
    apk = None
    try:
        t0 = time.perf_counter()
        apk = asvc.all_proofs_key(ctx, pk)
        key_ms = 1e3 * (time.perf_counter() - t0)
        runs, walls = [], []
        for _ in range(reps + 1):
            stats = {}
            t0 = time.perf_counter()
            xy, inf = asvc.prove_all(pk, apk, values, stats)
            walls.append(1e3 * (time.perf_counter() - t0))
            runs.append(stats)
        runs, walls = runs[1:], walls[1:]                          # the first run is the warm-up
        asvc.prove_pos(pk, values, [positions[0]])                 # warm-up
        singles, same = [], True
        for i in positions:
            t0 = time.perf_counter()
            p_xy, p_inf = asvc.prove_pos(pk, values, [i])
            singles.append(1e3 * (time.perf_counter() - t0))
            same = same and np.array_equal(p_xy, xy[i]) and bool(inf[i]) == p_inf
    finally:
        if apk is not None:
            apk.free()
        pk.free()
    single = float(np.median(singles))
    all_ms = float(np.median(walls))
    stages = ("upload", "ifft", "fft", "scale", "g1_ifft", "g1_fft", "download")
    pb = 16 * c.fq_limbs
    touched = 2 * n * (pb + 1) * 2 + 2 * n * 32                    # A and the work points with their flags, the scalars
    stage_bytes = 2 * (2 * n * (pb + 1)) * (log_n + 1) + 2 * (n * (pb + 1)) * log_n   # read + write per stage: 2n-point IFFT, n-point FFT
    gbs = ctx.bench_hbm_copy()
    return [dict(case="prove_all", curve=c.name, log_n=log_n, reps=reps, same_words_at_64_positions=bool(same),
                 prove_all_ms=round(all_ms, 3), prove_all_min_ms=round(min(walls), 3), prove_all_max_ms=round(max(walls), 3),
                 all_proofs_key_ms=round(key_ms, 3), **{s + "_ms": round(1e3 * float(np.median([r[s] for r in runs])), 3) for s in stages},
                 prove_pos_single_median_ms=round(single, 3), prove_pos_single_min_ms=round(min(singles), 3),
                 prove_pos_single_max_ms=round(max(singles), 3), n_times_single_ms=round(n * single, 1),
                 n_times_single_over_prove_all=round(n * single / all_ms, 1),
                 note="host wall time, every call ends in a synchronise; both sides include the integer -> Montgomery conversion of the values"),
            dict(case="copy_floor", curve=c.name, log_n=log_n, hbm_copy_gb_per_s=round(gbs, 1), buffers_touched_bytes=touched,
                 once_read_once_written_ms=round(2 * touched / gbs / 1e6, 4), butterfly_stage_bytes=stage_bytes,
                 stages_ms=round(stage_bytes / gbs / 1e6, 4), prove_all_over_stage_floor=round(all_ms / (stage_bytes / gbs / 1e6), 1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logs", type=int, nargs="*", default=[10, 13, 16])
    ap.add_argument("--compose-logs", type=int, nargs="*", default=[6, 7, 8, 9, 10])
    ap.add_argument("--prove-logs", type=int, nargs="*", default=[12, 16])
    ap.add_argument("--curves", nargs="*", default=["bn254", "bls12_381"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "asvc_all_bench.txt"))
    args = ap.parse_args()
    ctx = Context(0)                                               # no GPU: this raises
    reps = max(args.reps, 3)
    with open(args.out, "w") as f:
        def emit(line):
            text = json.dumps(line)
            print(text, flush=True)
            f.write(text + "\n")
            f.flush()

        for name in args.curves:
            c = get_curve(name)
            for log_n in args.logs:
                emit(ntt_case(ctx, c, log_n, reps))
            crossover = None
            for log_n in sorted(args.compose_logs):
                if log_n > 13:                                     # 32 n^2 bytes of scalars
                    continue
                line = composed_case(ctx, c, log_n, reps)
                emit(line)
                if crossover is None and line["composed_over_g1_ntt"] > 1:
                    crossover = log_n
            if args.compose_logs:
                emit(dict(case="crossover", curve=c.name, first_log_n_where_g1_ntt_wins=crossover, measured_logs=sorted(args.compose_logs),
                          note="null: the O(n^2) composition won at every measured size"))
            for log_n in args.prove_logs:
                for line in prove_case(ctx, c, log_n, reps):
                    emit(line)


if __name__ == "__main__":
    main()
