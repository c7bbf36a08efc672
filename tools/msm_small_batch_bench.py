#!/usr/bin/env python3
"""Batched small variable-base MSM (zkp_msm_g*_var_batch_dev) against a loop of zkp_msm_g*_var calls on the same inputs and, for
lone MSMs, against the resident-table zkp_msm_g1_dev.  HIP events around each call (zkp_timer_*), after warm-up; the median of
--reps.  One JSON line per case; every batched result is checked against the loop's (after normalisation to affine).

    python tools/msm_small_batch_bench.py [--reps 5]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import codec  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402
from oracle.pyref.curves import Group  # noqa: E402
from tests.util import OC, jac_limbs_to_affine_oracle, to_abi_points  # noqa: E402


def timed(ctx, fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        out = fn()
        ts.append(ctx.timer_stop_ms())
    return float(np.median(ts)), out


def case(ctx, curve, group, count, log_n, mont, reps, resident=False):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(count * 100 + log_n)
    d = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    g_xy, _ = to_abi_points(curve, group, [Group(OC[curve], group).gen])
    xy, inf = ctx.fixed_base_mul(c, group, g_xy, d)
    ks = []
    for _ in range(count):
        k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
        k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
        ks.append(codec.fr_to_mont(codec.limbs_to_ints(k), c) if mont else k)
    dxy, dinf = ctx.to_device(xy), ctx.to_device(inf)
    dks = [ctx.to_device(k) for k in ks]
    rec = {"case": f"{curve}_g{group}", "count": count, "log_n": log_n, "montgomery": mont}
    try:
        t_batch, out = timed(ctx, lambda: ctx.msm_var_batch_dev(c, group, [dxy] * count, [dinf] * count, dks, [n] * count, mont),
                             reps)
        t_loop, loop = timed(ctx, lambda: [ctx.msm_var(c, group, xy, inf, k, montgomery=mont) for k in ks], max(1, reps // 2))
        rec.update(batch_ms=round(t_batch, 4), var_loop_ms=round(t_loop, 4), speedup=round(t_loop / t_batch, 2))
        if resident:
            b = ctx.upload_bases(c, group, xy, inf)
            try:
                if mont:                                # zkp_msm_g1_mont_dev: Montgomery scalars on the device
                    res = np.zeros(3 * c.fq_limbs, dtype=np.uint64)
                    fn = lambda dk: ctx.lib.zkp_msm_g1_mont_dev(ctx.h, b.handle, 0, ctypes.c_void_p(dk), n,  # noqa: E731
                                                                ctypes.c_void_p(res.ctypes.data))
                else:
                    fn = lambda dk: b.msm_dev(dk, n)  # noqa: E731
                t_res, _ = timed(ctx, lambda: [fn(dk) for dk in dks], reps)
                rec["resident_dev_ms"] = round(t_res, 4)
            finally:
                b.free()
        rec["match"] = all(jac_limbs_to_affine_oracle(curve, group, out[i]) == jac_limbs_to_affine_oracle(curve, group, loop[i])
                           for i in range(count))
    finally:
        for p in [dxy, dinf] + dks:
            ctx.dev_free(p)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ok = True
    with Context(0) as ctx:
        for log_n in (10, 12, 14, 16):
            for mont in (False, True):
                ok &= case(ctx, "bn254", 1, 1, log_n, mont, a.reps, resident=True)["match"]
        ok &= case(ctx, "bn254", 1, 64, 10, False, a.reps)["match"]
        ok &= case(ctx, "bls12_381", 1, 16, 12, False, a.reps)["match"]
        ok &= case(ctx, "bn254", 2, 16, 12, False, a.reps)["match"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
