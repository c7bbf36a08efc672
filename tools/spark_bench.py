#!/usr/bin/env python3
"""SPARK memory-checking hashes and product circuits: the 12 "ops" circuits of a sparse-polynomial evaluation with three matrices
(6 lists, a read and a write circuit each) of n leaves.  HIP events around each call (zkp_timer_*), after warm-up; the median of
--reps (>= 20).  In one process, alternately, for every size:
  (a) zkp_fr_memcheck_circuits_dev: leaves, every layer and the roots in ceil((log2 n - 9) / 3) + 1 launches;
  (b) the same leaves and layers composed from zkp_fr_vec_op_dev, which is what a caller could do before: per list SCALE, AXPY, ADD,
      ADDC for the read leaves and ADDC for the write leaves (addr and ts already materialised as Fr vectors, outside the timing),
      then one MUL per layer and circuit: 30 + 12 log2 n launches;
  (c) the library's copy kernel (zkp_bench_hbm_copy) over the bytes (a) moves: the memory floor.
One JSON line per case.

    python tools/spark_bench.py [--reps 20] [--quick LOG_N]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import codec  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402
from ckb_zkp_amd.spark import layer_offset  # noqa: E402

VEC_MUL, VEC_ADD, VEC_SCALE, VEC_AXPY, VEC_ADDC = 0, 1, 3, 4, 5
LISTS = 6
TAIL_LOG = 9


def bytes_moved(log_n):
    """what (a) reads and writes: per list 40 B per leaf of inputs; per circuit every layer written once, and the input layer of
    every launch after the first read once"""
    n = 1 << log_n
    per_circuit = 32 * (2 * n - 2)
    length, rem = n, log_n - TAIL_LOG
    first = True
    while rem > 0:
        rl = min(rem, 3)
        if not first:
            per_circuit += 32 * length
        first = False
        length >>= rl
        rem -= rl
    if not first:
        per_circuit += 32 * length                                 # the tail reads its layer unless it is the only launch
    return LISTS * 40 * n + 2 * LISTS * per_circuit


def case(ctx, curve, log_n, reps, only_fused=False):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    host = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    host[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)   # any words below r are valid Montgomery elements for timing
    u32 = rng.integers(0, 1 << 28, size=n, dtype=np.uint32)
    bufs = []

    def alloc(nbytes):
        bufs.append(ctx.dev_alloc(nbytes))
        return bufs[-1]

    try:
        vals, addrs, tss = [], [], []
        for i in range(LISTS):
            v, a, t = alloc(32 * n), alloc(4 * n), alloc(4 * n)
            ctx.h2d(v, np.roll(host, 37 * i, axis=0))
            ctx.h2d(a, np.roll(u32, 11 * i))
            ctx.h2d(t, np.roll(u32, 13 * i + 5))
            vals.append(v), addrs.append(a), tss.append(t)
        circuits = [alloc(32 * (2 * n - 2)) for _ in range(2 * LISTS)]
        g1, g2 = codec.fr_to_mont([0x1234567 + log_n, 0x7654321], c)
        rep = lambda ps: [p for p in ps for _ in range(2)]         # noqa: E731
        fused = lambda: ctx.fr_memcheck_circuits_dev(c, rep(addrs), rep(vals), rep(tss), [0, 1] * LISTS, circuits, n, g1, g2)   # noqa: E731
        tag = {"curve": curve, "log_n": log_n, "circuits": 2 * LISTS}
        if only_fused:
            for _ in range(reps):
                fused()
            ctx.sync()
            return [dict(tag, case="fused_only", calls=reps, launches_per_call=max(0, (log_n - TAIL_LOG + 2) // 3) + 1)]
        # (b): addr and ts as Fr vectors (any Fr vector costs the same), a one-element slot for the root product
        addr_fr, ts_fr = alloc(32 * n), alloc(32 * n)
        ctx.h2d(addr_fr, np.roll(host, 101, axis=0))
        ctx.h2d(ts_fr, np.roll(host, 203, axis=0))
        slot = alloc(32)
        g1sq = codec.fr_to_mont([(0x1234567 + log_n) ** 2], c)[0]
        neg_g2, one = codec.fr_to_mont([c.r - 0x7654321, 1], c)

        def composed():
            for i in range(LISTS):
                rd, wr = circuits[2 * i], circuits[2 * i + 1]
                ctx.fr_vec_op(c, VEC_SCALE, addr_fr, None, rd, n, g1sq)
                ctx.fr_vec_op(c, VEC_AXPY, rd, vals[i], rd, n, g1)
                ctx.fr_vec_op(c, VEC_ADD, rd, ts_fr, rd, n)
                ctx.fr_vec_op(c, VEC_ADDC, rd, None, rd, n, neg_g2)
                ctx.fr_vec_op(c, VEC_ADDC, rd, None, wr, n, one)
            for p in circuits:
                for l in range(log_n):
                    half = n >> (l + 1)
                    src = p + 32 * layer_offset(n, l)
                    ctx.fr_vec_op(c, VEC_MUL, src, src + 32 * half, p + 32 * layer_offset(n, l + 1) if half > 1 else slot, half)
            ctx.sync()

        for _ in range(3):
            fused()
            composed()
        ta, tb = [], []
        for _ in range(reps):                                      # alternately, so that both see the same clocks
            ctx.timer_start()
            fused()
            ta.append(ctx.timer_stop_ms())
            ctx.timer_start()
            composed()
            tb.append(ctx.timer_stop_ms())
        ctx.sync()
        a_ms, b_ms = float(np.median(ta)), float(np.median(tb))
        moved = bytes_moved(log_n)
        gbs = ctx.bench_hbm_copy(max(moved // 2, 1 << 20))
        floor_ms = moved / (gbs * 1e9) * 1e3
        return [dict(tag, case="memcheck_circuits", fused_ms=round(a_ms, 4), fused_min_ms=round(float(np.min(ta)), 4),
                     composed_ms=round(b_ms, 4), composed_min_ms=round(float(np.min(tb)), 4), composed_over_fused=round(b_ms / a_ms, 2),
                     fused_launches=max(0, (log_n - TAIL_LOG + 2) // 3) + 1, composed_launches=5 * LISTS + 2 * LISTS * log_n,
                     bytes_moved=moved, gb_per_s=round(moved / (a_ms * 1e-3) / 1e9, 1), copy_gb_per_s=round(gbs, 1),
                     copy_floor_ms=round(floor_ms, 4), fused_over_floor=round(a_ms / floor_ms, 2),
                     leaves_per_us=round(2 * LISTS * n / (a_ms * 1e3), 1))]
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", type=int, default=0, metavar="LOG_N", help="BN254 at 2^LOG_N, three fused calls only (for a kernel trace)")
    ap.add_argument("--logs", default="12,16,20,24")
    args = ap.parse_args()
    ctx = Context(0)
    if args.quick:
        for line in case(ctx, "bn254", args.quick, 3, only_fused=True):
            print(json.dumps(line), flush=True)
        return
    for curve in ("bn254", "bls12_381"):
        for log_n in (int(x) for x in args.logs.split(",")):
            for line in case(ctx, curve, log_n, max(args.reps, 20)):
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
