#!/usr/bin/env python3
"""zkp_fr_asvc_quotient_dev against its composition from the exports that existed before it: k successive zkp_poly_div_linear_dev
calls (five launches each, no read-back) on ping-pong buffers.  HIP events around each alternative (zkp_timer_*), every window
ends in a synchronise; after a warm-up the alternatives take turns inside one loop of one process, the composition twice per turn
(composed / composed_again: the spread between two runs of the same work).  Both are checked to give the same words at every timed
size.  One JSON line per (n, k):
  * products_per_pair: the Fr products the fused chain performs per (coefficient, position), from its structure: (L - 1) / L in the
    segment-head pass, 1 (L >= 8) or (L - 1) / L in the output pass, and (3 + 29 / 32) / L in the scan over n k / L heads
    (chunk head 1, replay 2, tile scan and carry 29 per 32-head chunk), L = 2^floor(log2 k); the composition performs about 3.2 per factor (chunk 1, replay 1,
    tile scan 1 / 2, the fix pass and the powers of z about 0.7);
  * gproducts_per_s: n k products_per_pair / time, against zkp_bench_mulmod's sustained rate from the same run;
  * verdict: "faster" / "slower" only when the difference exceeds the composition's own spread, else "within spread".
Then the per-stage split of asvc.prove_pos at --prove-log (host wall time, every stage ends in a synchronise).

    python tools/asvc_bench.py [--reps 5] [--logs 16 20 24] [--ks 1 4 16 64 256 1024] [--prove-log 20] [--curve bn254]
Runs on the GPU only: creating the context fails without one."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import _lib, asvc, codec  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402


def rand_fr(rng, c, n):
    """n reduced values as Montgomery words (any words below r are a valid vector)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def products_per_pair(k: int) -> float:
    seg = asvc.segment_length(k)
    return (seg - 1) / seg + (1.0 if seg >= asvc.ASVC_SPAN else (seg - 1) / seg) + (3 + 29 / 32) / seg


def read(ctx, ptr, n):
    a = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(a, ptr)
    return a


def quotient_case(ctx, c, log_n, k, reps, d_phi, bufs, ceiling):
    n = 1 << log_n
    rng = np.random.default_rng(1000 * log_n + k)
    points = [int(p) for p in rng.choice(n, size=k, replace=False)]
    w = asvc.domain_root(c, n)
    roots = codec.fr_to_mont([pow(w, p, c.r) for p in points], c)
    d_q, d_a, d_b = bufs

    def fused():
        ctx.fr_asvc_quotient_dev(c, d_phi, log_n, points, d_q)

    def composed():
        src, length, dst = d_phi, n, d_a
        for i in range(k):
            _lib.check(ctx.lib.zkp_poly_div_linear_dev(ctx.h, c.cid, C.c_void_p(src), length, C.c_void_p(roots[i].ctypes.data),
                                                       C.c_void_p(dst), None), "zkp_poly_div_linear_dev")
            src, length, dst = dst, length - 1, (d_b if dst == d_a else d_a)
        ctx.sync()
        return src

    fused()
    last = composed()
    same = bool(np.array_equal(read(ctx, d_q, n - k), read(ctx, last, n - k)))
    fns = {"fused": fused, "composed": composed, "composed_again": composed}
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ctx.timer_start()
            fn()
            ts[name].append(ctx.timer_stop_ms())
    med = {name: float(np.median(v)) for name, v in ts.items()}
    spread = abs(med["composed"] - med["composed_again"])
    comp = min(med["composed"], med["composed_again"])
    verdict = "within spread" if abs(med["fused"] - comp) <= spread else ("faster" if med["fused"] < comp else "slower")
    ppp = products_per_pair(k)
    rate = n * k * ppp / (med["fused"] * 1e-3) / 1e9
    line = dict(case="quotient", curve=c.name, log_n=log_n, k=k, same_words=same, reps=reps, launches=dict(fused=9, composed=5 * k),
                fused_ms=round(med["fused"], 4), composed_ms=round(med["composed"], 4), composed_again_ms=round(med["composed_again"], 4),
                fused_min_ms=round(min(ts["fused"]), 4), composed_min_ms=round(min(ts["composed"] + ts["composed_again"]), 4),
                spread_ms=round(spread, 4), composed_over_fused=round(comp / med["fused"], 2), verdict=verdict,
                products_per_pair=round(ppp, 3), gproducts_per_s=round(rate, 1), mulmod_ceiling_gproducts_per_s=round(ceiling, 1),
                of_ceiling=round(rate / ceiling, 3))
    return line


def prove_case(ctx, c, log_n, k, reps):
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    gen_xy, _ = codec.g1_to_mont([c.g1], c)
    tau = 0x1234567890ABCDEF1234567890ABCDEF
    powers = codec.fr_canonical([pow(tau, j, c.r) for j in range(n + 1)], c)
    p1, _ = ctx.fixed_base_mul(c, 1, gen_xy[0], powers)
    pk = asvc.ProvingKey(c, n, p1, p1[:n], p1[:n], p1[:n]).upload(ctx)            # prove_pos reads powers_of_g1 only
    values = codec.fr_from_mont(rand_fr(rng, c, n), c)
    points = [int(p) for p in rng.choice(n, size=k, replace=False)]
    try:
        runs = []
        for _ in range(reps + 1):
            stats = {}
            asvc.prove_pos(pk, values, points, stats)
            runs.append(stats)
    finally:
        pk.free()
    runs = runs[1:]                                                # the first run is the warm-up
    stages = ("upload", "ifft", "quotient", "msm", "affine")
    return dict(case="prove_pos", curve=c.name, log_n=log_n, k=k, reps=reps,
                **{s + "_ms": round(1e3 * float(np.median([r[s] for r in runs])), 3) for s in stages},
                note="host wall time per stage, each ending in a synchronise; upload includes the integer -> Montgomery conversion")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logs", type=int, nargs="*", default=[16, 20, 24])
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 4, 16, 64, 256, 1024])
    ap.add_argument("--prove-log", type=int, default=20)
    ap.add_argument("--prove-k", type=int, default=16)
    ap.add_argument("--curve", default="bn254")
    args = ap.parse_args()
    ctx = Context(0)                                               # no GPU: this raises
    c = get_curve(args.curve)
    reps = max(args.reps, 3)
    ceiling = ctx.bench_mulmod(c, 0, False)
    for log_n in args.logs:
        n = 1 << log_n
        rng = np.random.default_rng(log_n)
        d_phi = ctx.to_device(rand_fr(rng, c, n))
        bufs = [ctx.dev_alloc(32 * n) for _ in range(3)]
        try:
            for k in args.ks:
                if k <= n:
                    print(json.dumps(quotient_case(ctx, c, log_n, k, reps, d_phi, bufs, ceiling)), flush=True)
        finally:
            ctx.sync()
            for p in [d_phi] + bufs:
                ctx.dev_free(p)
    if args.prove_log:
        print(json.dumps(prove_case(ctx, c, args.prove_log, args.prove_k, reps)), flush=True)


if __name__ == "__main__":
    main()
