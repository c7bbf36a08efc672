#!/usr/bin/env python3
"""zkp_pairing_miller_dev / zkp_pairing_final_exp_dev and the Groth16 batch verifier, measured.  One JSON line per case, per curve:

  * miller at --logs: n pairs in ONE group (the shape of a batch verifier: n Miller loops, one product), HIP events around the call
    (zkp_timer_*), median of --reps after one warm-up: Miller loops per second;
  * final_exp at the same sizes: n elements (the Miller values of the n pairs, group 1), in place, the same timing: final
    exponentiations per second;
  * both against the multiplier: the Fq products of the formulas (pairing.FQ_PRODUCTS: counted by running csrc/pairing_dev.hpp on a
    CPU field, tests/test_pairing_ref.py; + 54 per pair for the product tree) times the measured rate, over zkp_bench_mulmod's Fq
    rate of the same run (the saturated multiplier, the one this unit calls) = the fraction of the multiplier's rate that the kernels
    reach;
  * groth16_batch: verify_proofs_batch over --proofs Mini proofs (host wall time, it ends in a synchronise; the host work of
    encoding points is inside) against --proofs calls of verify_proof, each the median of 3 / one pass.

    python tools/pairing_bench.py [--reps 5] [--logs 6 10 14 16] [--proofs 1024] [--curves bn254 bls12_381]
                                  [--out profiles/pairing_bench.txt]
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

from ckb_zkp_amd import codec, groth16  # noqa: E402
from ckb_zkp_amd import pairing as zp  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.circuits import Mini  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402

TOXIC = dict(alpha=0x1234567890ABCDEF1, beta=0xFEDCBA09876543211, gamma=0x1111111111111111111,
             delta=0x2222222222222222223, tau=0x3333333333333333335)


def rand_fr(rng, c, n):
    """n reduced values as words (any words below r are a valid vector)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def timed(ctx, fn, reps):
    fn()                                                           # warm-up
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop_ms())
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def kernel_case(ctx, c, log_n, reps, fq_rate):
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    g1, i1 = ctx.fixed_base_mul(c, 1, codec.g1_to_mont([c.g1], c)[0][0], rand_fr(rng, c, n))
    g2, i2 = ctx.fixed_base_mul(c, 2, codec.g2_to_mont([c.g2], c)[0][0], rand_fr(rng, c, n))
    w = 12 * c.fq_limbs
    bufs = [ctx.to_device(a) for a in (g1, i1, g2, i2)] + [ctx.dev_alloc(n * w * 8), ctx.dev_alloc(n * w * 8)]
    d1, e1, d2, e2, d_one, d_all = bufs
    cnt = zp.FQ_PRODUCTS[c.name]
    out = []
    try:
        ms, lo, hi = timed(ctx, lambda: ctx.pairing_miller_dev(c, d1, e1, d2, e2, n, n, d_one), reps)
        per_s = n / (ms * 1e-3)
        products = cnt["miller"] + zp.FQ12_MUL_PRODUCTS
        out.append(dict(case="miller", curve=c.name, log_n=log_n, group=n, reps=reps, ms=round(ms, 3), min_ms=round(lo, 3),
                        max_ms=round(hi, 3), miller_loops_per_s=round(per_s), fq_products_per_loop=products,
                        fq_products_per_s=round(per_s * products), fq_mulmod_per_s=round(fq_rate * 1e9),
                        fraction_of_mulmod=round(per_s * products / (fq_rate * 1e9), 4)))
        ctx.pairing_miller_dev(c, d1, e1, d2, e2, n, 1, d_all)        # n Miller values: the inputs of the final exponentiation
        ctx.sync()
        ms, lo, hi = timed(ctx, lambda: ctx.pairing_final_exp_dev(c, d_all, n, d_all), reps)   # GT values are valid inputs too
        per_s = n / (ms * 1e-3)
        out.append(dict(case="final_exp", curve=c.name, log_n=log_n, reps=reps, ms=round(ms, 3), min_ms=round(lo, 3),
                        max_ms=round(hi, 3), final_exps_per_s=round(per_s), fq_products_per_exp=cnt["final_exp"],
                        fq_products_per_s=round(per_s * cnt["final_exp"]), fq_mulmod_per_s=round(fq_rate * 1e9),
                        fraction_of_mulmod=round(per_s * cnt["final_exp"] / (fq_rate * 1e9), 4)))
    finally:
        for p in bufs:
            ctx.dev_free(p)
    return out


def groth16_case(ctx, c, n):
    rng = random.Random(n)
    params = groth16.generate_parameters(ctx, c, Mini(num=10), **TOXIC)
    pk = groth16.ProvingKey(ctx, params, Mini(num=10))
    proofs, inputs = [], []
    try:
        for _ in range(n):
            x, y = rng.randrange(1, c.r), rng.randrange(1, c.r)
            z = x * (y + 2) % c.r
            proofs.append(groth16.create_proof(pk, Mini(x, y, z, 10), rng.randrange(c.r), rng.randrange(c.r)))
            inputs.append([z])
    finally:
        pk.free()
    pvk = groth16.prepare_verifying_key(ctx, params)
    rho = groth16.batch_coefficients(c, n, seed=1)
    assert groth16.verify_proofs_batch(ctx, pvk, proofs, inputs, rho)          # warm-up
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ok = groth16.verify_proofs_batch(ctx, pvk, proofs, inputs, rho)
        ts.append(time.perf_counter() - t0)
        assert ok
    batch_s = float(np.median(ts))
    assert groth16.verify_proof(ctx, pvk, proofs[0], inputs[0])                # warm-up
    t0 = time.perf_counter()
    for p, x in zip(proofs, inputs):
        assert groth16.verify_proof(ctx, pvk, p, x)
    single_s = time.perf_counter() - t0
    return dict(case="groth16_batch", curve=c.name, proofs=n, verify_proofs_batch_s=round(batch_s, 4),
                verify_proof_calls_s=round(single_s, 4), per_proof_ms_batch=round(1e3 * batch_s / n, 4),
                per_proof_ms_single=round(1e3 * single_s / n, 4), single_over_batch=round(single_s / batch_s, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logs", type=int, nargs="*", default=[6, 10, 14, 16])
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--curves", nargs="*", default=["bn254", "bls12_381"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    with Context(0) as ctx:
        for name in args.curves:
            c = get_curve(name)
            fq_rate = ctx.bench_mulmod(c, 1, False)
            emit(dict(case="info", curve=c.name, fq_mulmod_g_per_s=round(fq_rate, 2), **ctx.pairing_info(c)))
            for log_n in args.logs:
                for d in kernel_case(ctx, c, log_n, args.reps, fq_rate):
                    emit(d)
            if args.proofs:
                emit(groth16_case(ctx, c, args.proofs))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
