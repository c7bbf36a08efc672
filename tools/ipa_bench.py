#!/usr/bin/env python3
"""IPA generator fold (zkp_g1_ipa_fold_dev), batched Fr inner products (zkp_fr_dot_batch_dev) and the whole device IPA prover
(ipa.inner_product_prove).  HIP events around each call (zkp_timer_*), after one warm-up call; the median of --reps.  One JSON line
per case.  For the fold: points/s, and the ESTIMATED Fq products of one point (131 doublings x 9 + 131 additions x 14 + the table
and the affine tail, ~3 100) times the points over the time, against zkp_bench_mulmod's unsaturated Fq rate.

    python tools/ipa_bench.py [--reps 5] [--quick]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import codec, ipa  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402
from oracle.pyref.curves import Group  # noqa: E402
from tests.util import OC, to_abi_points  # noqa: E402

EST_PRODUCTS = 131 * 9 + 131 * 14 + 14 + 4 + 10        # estimate per point, not a count


def timed(ctx, fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop_ms())
    return float(np.median(ts))


def rand_fr(rng, c, n):
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def points(ctx, curve, n, seed):
    c = get_curve(curve)
    g_xy, _ = to_abi_points(curve, 1, [Group(OC[curve], 1).gen])
    return ctx.fixed_base_mul(c, 1, g_xy, rand_fr(np.random.default_rng(seed), c, n))


def fold_case(ctx, curve, log_n, reps, rate):
    c = get_curve(curve)
    n = 1 << log_n
    xy, inf = points(ctx, curve, 2 * n, log_n)
    rng = np.random.default_rng(7)
    a, b = codec.fr_to_mont(codec.limbs_to_ints(rand_fr(rng, c, 2)), c)
    d = ctx.to_device(xy)
    di = ctx.to_device(inf)
    do = ctx.dev_alloc(xy.nbytes // 2)
    doi = ctx.dev_alloc(n)
    ab = xy.shape[1] * 8
    try:
        ms = timed(ctx, lambda: ctx.ipa_fold_dev(c, d, di, d + n * ab, di + n, n, a, b, do, doi), reps)
    finally:
        for p in (d, di):
            ctx.dev_free(p)
        ctx.dev_free(do)
        ctx.dev_free(doi)
    est = EST_PRODUCTS * n / (ms * 1e-3) / 1e9
    return {"case": f"fold_{curve}_g1", "log_n": log_n, "ms": round(ms, 4), "points_per_s": round(n / (ms * 1e-3)),
            "est_gproducts_per_s": round(est, 1), "mulmod_roof_gproducts_per_s": round(rate, 1),
            "fraction_of_roof": round(est / rate, 3)}


def dot_case(ctx, curve, count, log_n, reps):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(3)
    A = codec.fr_to_mont(codec.limbs_to_ints(rand_fr(rng, c, n)), c)
    da = ctx.to_device(A)
    try:
        ms = timed(ctx, lambda: ctx.fr_dot_batch_dev(c, [da] * count, [da] * count, [n] * count), reps)
    finally:
        ctx.dev_free(da)
    return {"case": f"fr_dot_batch_{curve}", "count": count, "log_n": log_n, "ms": round(ms, 4),
            "terms_per_s": round(count * n / (ms * 1e-3))}


def prove_case(ctx, curve, log_n, reps):
    c = get_curve(curve)
    n = 1 << log_n
    g_xy, g_inf = points(ctx, curve, n, 100 + log_n)
    qh, _ = points(ctx, curve, 2, 5)
    rng = np.random.default_rng(9)
    m = lambda k: codec.fr_to_mont(codec.limbs_to_ints(k), c)        # noqa: E731
    a, b, gb = m(rand_fr(rng, c, n)), m(rand_fr(rng, c, n)), m(rand_fr(rng, c, 1))[0]
    blinds = [tuple(m(rand_fr(rng, c, 2))) for _ in range(log_n)]

    def ch(l_xy, l_inf, r_xy, r_inf):
        h = hashlib.sha256(l_xy.tobytes() + bytes([int(l_inf)]) + r_xy.tobytes() + bytes([int(r_inf)])).digest()
        return int.from_bytes(h, "little") % c.r or 1

    ms = timed(ctx, lambda: ipa.inner_product_prove(ctx, c, g_xy, g_inf, qh[0], qh[1], a, b, gb, blinds, ch), reps)
    return {"case": f"inner_product_prove_{curve}", "log_n": log_n, "ms": round(ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the whole prover only (for a kernel trace)")
    args = ap.parse_args()
    ctx = Context(0)
    if args.quick:
        print(json.dumps(prove_case(ctx, "bn254", 14, 1)), flush=True)
        return
    for curve, top in (("bn254", 20), ("bls12_381", 18)):
        rate = ctx.bench_mulmod(curve, 1, True)
        for log_n in range(10, top + 1):
            print(json.dumps(fold_case(ctx, curve, log_n, args.reps, rate)), flush=True)
    for count, log_n in ((2, 10), (2, 15), (2, 20), (64, 12)):
        print(json.dumps(dot_case(ctx, "bn254", count, log_n, args.reps)), flush=True)
    for log_n in (10, 14, 16):
        print(json.dumps(prove_case(ctx, "bn254", log_n, args.reps)), flush=True)


if __name__ == "__main__":
    main()
