#!/usr/bin/env python3
"""PLONK rounds 2 and 3 on the device: the running product (zkp_fr_prefix_product_dev), the permutation accumulator
(zkp_fr_plonk_perm_z_dev), the fused quotient (zkp_fr_plonk_quotient_dev) and rounds 1-3 of ckb_zkp_amd.plonk.  HIP events around
each call (zkp_timer_*), after warm-up; the median of --reps (>= 20); the alternatives of a comparison take turns inside one loop
of one process.  One JSON line per case.  Each call is timed against
  (a) its composition from the exports that existed before it: zkp_fr_vec_op_dev, zkp_fr_batch_inverse_dev and zkp_d2d over
      device tables of w^i / g w^i / v_4n_inversed that are built before the clock starts; the running product (also inside the
      composed z) is a host loop over one download, timed by the host clock with --reps-host repetitions;
  (b) the library's copy kernel (zkp_bench_hbm_copy) over the bytes the call must move: 2 vectors for the product, 8 + 1 for z,
      18 + 1 for the quotient.
  (c) rounds 1-3 (plonk.prover_first_round .. prover_third_round, coefficient vectors left on the device) at 2^20 rows.

    python tools/plonk_bench.py [--reps 20] [--logs 12 14 ..] [--quick] [--only a|c]
--quick: 2^12, each call exactly once and nothing else (for a kernel trace that counts launches).
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
from ckb_zkp_amd.api import NTT_COSET_FFT, NTT_FFT, Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402

VEC_MUL, VEC_ADD, VEC_SUB, VEC_SCALE, VEC_AXPY, VEC_ADDC = 0, 1, 2, 3, 4, 5
KS = [1, 7, 13, 17]


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


def powers_table(ctx, c, log_size, coset):
    """w^i (or g w^i) over the domain of 2^log_size points as a device table: the transform of the polynomial X"""
    size = 1 << log_size
    x = np.zeros((size, 4), dtype=np.uint64)
    x[1] = codec.fr_mont(1, c)
    d = ctx.to_device(x)
    ctx.ntt_dev(c, d, log_size, NTT_COSET_FFT if coset else NTT_FFT)
    return d


def host_prefix_product(ctx, c, d_in, d_out, n):
    """the running product as a host loop over one download"""
    a = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(a, d_in)
    r, ri = c.r, pow(1 << 256, -1, c.r)
    acc, out = (1 << 256) % r, []
    for v in codec.limbs_to_ints(a):
        out.append(acc)
        acc = acc * v % r * ri % r
    ctx.h2d(d_out, codec.ints_to_limbs(out, 4))
    return acc


def read(ctx, d, n):
    a = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(a, d)
    return a


# ------------------------------------------------------------------------------------------- the three calls
def product_case(ctx, curve, log_n, reps, reps_host):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(log_n)
    d_in, d_a, d_b = ctx.to_device(rand_fr(rng, c, n)), ctx.dev_alloc(32 * n), ctx.dev_alloc(32 * n)
    try:
        t = timed_alternating(ctx, {"device": lambda: ctx.fr_prefix_product_dev(c, d_in, d_a, n)}, reps)
        host = timed_host(ctx, lambda: host_prefix_product(ctx, c, d_in, d_b, n), reps_host)
        same = bool(np.array_equal(read(ctx, d_a, n), read(ctx, d_b, n)))
        moved = 64 * n
        gbs, fl = floor_ms(ctx, moved)
        levels = 0 if n <= plonk.PLONK_SCAN_BLOCK else 1 if n <= plonk.PLONK_SCAN_BLOCK ** 2 else 2
        return [dict(case="prefix_product", curve=curve, log_n=log_n, launches=1 + 2 * levels, device_ms=round(t["device"][0], 4),
                     device_min_ms=round(t["device"][1], 4), host_loop_ms=round(host[0], 2), host_loop_min_ms=round(host[1], 2),
                     host_reps=reps_host, host_over_device=round(host[0] / t["device"][0], 1), same_result=same, bytes_moved=moved,
                     copy_gb_per_s=round(gbs, 1), copy_floor_ms=round(fl, 4), device_over_floor=round(t["device"][0] / fl, 2))]
    finally:
        ctx.sync()
        for p in (d_in, d_a, d_b):
            ctx.dev_free(p)


def composed_perm_terms(ctx, c, w, sigma, roots, kb, beta, gamma, n, num, den, tmp):
    """perm[i] into num from vector ops and one batch inversion: 24 launches"""
    for j in range(4):
        ctx.fr_vec_op(c, VEC_AXPY, w[j], roots, tmp, n, kb[j])              # w_j + ks_j beta w^i
        ctx.fr_vec_op(c, VEC_ADDC, tmp, None, tmp if j else num, n, gamma)
        if j:
            ctx.fr_vec_op(c, VEC_MUL, num, tmp, num, n)
    for j in range(4):
        ctx.fr_vec_op(c, VEC_AXPY, w[j], sigma[j], tmp, n, beta)            # w_j + beta sigma_j
        ctx.fr_vec_op(c, VEC_ADDC, tmp, None, tmp if j else den, n, gamma)
        if j:
            ctx.fr_vec_op(c, VEC_MUL, den, tmp, den, n)
    ctx.fr_batch_inverse(c, den, n)
    ctx.fr_vec_op(c, VEC_MUL, num, den, num, n)


def perm_z_case(ctx, curve, log_n, reps, reps_host):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(100 + log_n)
    host = rand_fr(rng, c, n)
    w = [ctx.to_device(np.roll(host, 11 * j, axis=0)) for j in range(4)]
    sigma = [ctx.to_device(np.roll(host, 5 + 13 * j, axis=0)) for j in range(4)]
    roots = powers_table(ctx, c, log_n, False)
    z_a, z_b, num, den, tmp = (ctx.dev_alloc(32 * n) for _ in range(5))
    beta_i, gamma_i = 0x1234567 + log_n, 0x7654321
    ks, beta, gamma = codec.fr_to_mont(KS, c), codec.fr_mont(beta_i, c), codec.fr_mont(gamma_i, c)
    kb = [codec.fr_mont(k * beta_i, c) for k in KS]
    try:
        terms = lambda: composed_perm_terms(ctx, c, w, sigma, roots, kb, beta, gamma, n, num, den, tmp)    # noqa: E731
        t = timed_alternating(ctx, {"fused": lambda: ctx.fr_plonk_perm_z_dev(c, w, sigma, log_n, ks, beta, gamma, z_a),
                                    "composed_terms": terms}, reps)
        host_t = timed_host(ctx, lambda: (terms(), host_prefix_product(ctx, c, num, z_b, n)), reps_host)
        same = bool(np.array_equal(read(ctx, z_a, n), read(ctx, z_b, n)))
        moved = 9 * 32 * n
        gbs, fl = floor_ms(ctx, moved)
        return [dict(case="perm_z", curve=curve, log_n=log_n, fused_ms=round(t["fused"][0], 4), fused_min_ms=round(t["fused"][1], 4),
                     composed_terms_ms=round(t["composed_terms"][0], 4), composed_terms_launches=24,
                     composed_with_host_product_ms=round(host_t[0], 2), host_reps=reps_host,
                     composed_terms_over_fused=round(t["composed_terms"][0] / t["fused"][0], 2),
                     composed_over_fused=round(host_t[0] / t["fused"][0], 1), same_result=same, bytes_moved=moved,
                     copy_gb_per_s=round(gbs, 1), copy_floor_ms=round(fl, 4), fused_over_floor=round(t["fused"][0] / fl, 2))]
    finally:
        ctx.sync()
        for p in w + sigma + [roots, z_a, z_b, num, den, tmp]:
            ctx.dev_free(p)


def composed_quotient(ctx, c, t, xs, vinv, k, N, out, tmp):
    """the quotient from vector ops and two copies: 46 launches.  t: name -> device table; k: the Montgomery constants"""
    a, num, den, zn, s = tmp
    op = ctx.fr_vec_op
    op(c, VEC_MUL, t["q_0"], t["w_0"], a, N)
    for j in (1, 2, 3):
        op(c, VEC_MUL, t[f"q_{j}"], t[f"w_{j}"], s, N)
        op(c, VEC_ADD, a, s, a, N)
    op(c, VEC_MUL, t["q_m"], t["w_1"], s, N)
    op(c, VEC_MUL, s, t["w_2"], s, N)
    op(c, VEC_ADD, a, s, a, N)
    op(c, VEC_ADD, a, t["q_c"], a, N)
    op(c, VEC_ADD, a, t["pi"], a, N)
    op(c, VEC_MUL, a, t["q_arith"], a, N)
    ctx.d2d(zn, t["z"] + 32 * 4, 32 * (N - 4))                              # z one row on, wrapping
    ctx.d2d(zn + 32 * (N - 4), t["z"], 32 * 4)
    for j in range(4):
        op(c, VEC_AXPY, t[f"w_{j}"], xs, s, N, k["kb"][j])
        op(c, VEC_ADDC, s, None, s, N, k["gamma"])
        op(c, VEC_MUL, num if j else t["z"], s, num, N)
    for j in range(4):
        op(c, VEC_AXPY, t[f"w_{j}"], t[f"sigma_{j}"], s, N, k["beta"])
        op(c, VEC_ADDC, s, None, s, N, k["gamma"])
        op(c, VEC_MUL, den if j else zn, s, den, N)
    op(c, VEC_SUB, num, den, num, N)
    op(c, VEC_SCALE, num, None, num, N, k["alpha"])
    op(c, VEC_ADDC, t["z"], None, s, N, k["minus_one"])
    op(c, VEC_MUL, s, t["l1"], s, N)
    op(c, VEC_AXPY, a, s, a, N, k["alpha2"])
    op(c, VEC_ADD, a, num, a, N)
    op(c, VEC_MUL, a, vinv, out, N)


TABLES = ["w_0", "w_1", "w_2", "w_3", "z", "pi", "q_0", "q_1", "q_2", "q_3", "q_m", "q_c", "q_arith", "sigma_0", "sigma_1", "sigma_2",
          "sigma_3", "l1"]


def quotient_case(ctx, curve, log_n, reps):
    c = get_curve(curve)
    N = 4 << log_n
    rng = np.random.default_rng(200 + log_n)
    host = rand_fr(rng, c, N)
    t = {name: ctx.to_device(np.roll(host, 7 * i, axis=0)) for i, name in enumerate(TABLES)}
    xs = powers_table(ctx, c, log_n + 2, True)
    # v_4n_inversed as the reference builds it: the coset transform of X^n - 1, inverted point by point
    v = np.zeros((N, 4), dtype=np.uint64)
    v[0], v[1 << log_n] = codec.fr_mont(c.r - 1, c), codec.fr_mont(1, c)
    vinv = ctx.to_device(v)
    ctx.ntt_dev(c, vinv, log_n + 2, NTT_COSET_FFT)
    ctx.fr_batch_inverse(c, vinv, N)
    out_a, out_b = ctx.dev_alloc(32 * N), ctx.dev_alloc(32 * N)
    tmp = [ctx.dev_alloc(32 * N) for _ in range(5)]
    b, g, al = 0x1234567 + log_n, 0x7654321, 0xABCDEF01
    k = dict(kb=[codec.fr_mont(x * b, c) for x in KS], beta=codec.fr_mont(b, c), gamma=codec.fr_mont(g, c), alpha=codec.fr_mont(al, c),
             alpha2=codec.fr_mont(al * al, c), minus_one=codec.fr_mont(c.r - 1, c))
    ks = codec.fr_to_mont(KS, c)
    try:
        fused = lambda: ctx.fr_plonk_quotient_dev(c, [t[f"w_{j}"] for j in range(4)], t["z"], t["pi"], [t[q] for q in TABLES[6:13]],   # noqa: E731
                                                  [t[s] for s in TABLES[13:17]], t["l1"], log_n, ks, k["beta"], k["gamma"], k["alpha"], out_a)
        tm = timed_alternating(ctx, {"fused": fused, "composed": lambda: composed_quotient(ctx, c, t, xs, vinv, k, N, out_b, tmp)}, reps)
        same = bool(np.array_equal(read(ctx, out_a, N), read(ctx, out_b, N)))
        moved = 19 * 32 * N
        gbs, fl = floor_ms(ctx, moved)
        return [dict(case="quotient", curve=curve, log_n=log_n, points=N, fused_ms=round(tm["fused"][0], 4), fused_min_ms=round(tm["fused"][1], 4),
                     composed_ms=round(tm["composed"][0], 4), composed_min_ms=round(tm["composed"][1], 4), composed_launches=46,
                     composed_over_fused=round(tm["composed"][0] / tm["fused"][0], 2), same_result=same, bytes_moved=moved,
                     copy_gb_per_s=round(gbs, 1), copy_floor_ms=round(fl, 4), fused_over_floor=round(tm["fused"][0] / fl, 2))]
    finally:
        ctx.sync()
        for p in list(t.values()) + [xs, vinv, out_a, out_b] + tmp:
            ctx.dev_free(p)


# ------------------------------------------------------------------------------------------- rounds 1-3
def rounds_case(ctx, curve, log_n, reps):
    """a circuit whose copy constraints are the identity (sigma_j = ks_j w^i: every witness closes) with random selector and
    witness words: the time of a round does not depend on the values"""
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(300 + log_n)
    roots = powers_table(ctx, c, log_n, False)
    tmp = ctx.dev_alloc(32 * n)
    sel = {"n": n}
    for j in range(4):
        ctx.fr_vec_op(c, VEC_SCALE, roots, None, tmp, n, codec.fr_mont(KS[j], c))
        sel[f"sigma_{j}"] = read(ctx, tmp, n)
    for p in (roots, tmp):
        ctx.dev_free(p)
    host = rand_fr(rng, c, n)
    for i, name in enumerate(plonk.SELECTORS[:7]):
        sel[name] = np.roll(host, 3 * i, axis=0)
    t0 = time.perf_counter()
    ix = plonk.Index(ctx, c, sel, KS)
    index_ms = (time.perf_counter() - t0) * 1e3
    ps = plonk.prover_init(ix, np.roll(host, 101, axis=0))
    w = [np.roll(host, 17 * (j + 1), axis=0) for j in range(4)]
    try:
        def rounds():
            plonk.prover_first_round(ps, w, to_host=False)
            plonk.prover_second_round(ps, 0x1234567, 0x7654321, to_host=False)
            plonk.prover_third_round(ps, 0xABCDEF01, to_host=False)

        rounds()                                                       # warm-up: twiddle tables, scratch, code objects
        whole = timed_host(ctx, rounds, reps)
        parts = {}
        for name, fn in (("round1", lambda: plonk.prover_first_round(ps, w, to_host=False)),
                         ("round2", lambda: plonk.prover_second_round(ps, 0x1234567, 0x7654321, to_host=False)),
                         ("round3", lambda: plonk.prover_third_round(ps, 0xABCDEF01, to_host=False))):
            parts[name] = round(timed_host(ctx, fn, reps)[0], 2)
        return [dict(case="rounds_1_3", curve=curve, log_n=log_n, ms=round(whole[0], 2), min_ms=round(whole[1], 2), reps=reps, **parts,
                     index_ms=round(index_ms, 1),
                     note="host clock around rounds that end in a synchronise; round 1 includes the upload of 4 witness vectors")]
    finally:
        ps.close()
        ix.close()


def quick(ctx):
    """2^12: one call of every kind, no warm-up, so that a kernel trace shows the launches per call"""
    c = get_curve("bn254")
    log_n = 12
    n, N = 1 << log_n, 4 << log_n
    rng = np.random.default_rng(1)
    host = rand_fr(rng, c, N)
    d = [ctx.to_device(np.roll(host, 3 * i, axis=0)) for i in range(19)]
    one = codec.fr_mont(1, c)
    ks = codec.fr_to_mont(KS, c)
    ctx.fr_prefix_product_dev(c, d[0], d[18], 1000)
    ctx.fr_prefix_product_dev(c, d[0], d[18], n)
    ctx.fr_plonk_perm_z_dev(c, d[0:4], d[4:8], log_n, ks, one, one, d[18])
    ctx.fr_plonk_quotient_dev(c, d[0:4], d[4], d[5], d[6:13], d[13:17], d[17], log_n, ks, one, one, one, d[18])
    ctx.sync()
    for p in d:
        ctx.dev_free(p)
    plan = ["prefix_product, 1000 elements: 1 launch", "prefix_product, 2^12 elements: 3 launches",
            "perm_z, 2^12 rows: 1 (terms) + 1 (batch inverse) + 3 (product) launches", "quotient, 2^14 points: 1 launch"]
    print(json.dumps(dict(case="quick", calls=plan, expected_kernel_calls=dict(scan_apply_kernel=5, scan_totals_kernel=2, perm_terms_kernel=1,
                                                                              batch_inverse_kernel=1, quotient_kernel=1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-host", type=int, default=2, help="repetitions of the host-loop alternatives (seconds each at 2^22)")
    ap.add_argument("--reps-whole", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="2^12 BN254, one call of every kind (for a kernel trace)")
    ap.add_argument("--only", choices=["a", "c"], default=None)
    ap.add_argument("--logs", type=int, nargs="*", default=None, help="log2 of the rows instead of 12, 14, .., 22")
    ap.add_argument("--curves", nargs="*", default=["bn254", "bls12_381"])
    args = ap.parse_args()
    ctx = Context(0)
    if args.quick:
        return quick(ctx)
    reps = max(args.reps, 20)
    emit = lambda lines: [print(json.dumps(line), flush=True) for line in lines]    # noqa: E731
    if args.only in (None, "a"):
        for curve in args.curves:
            for log_n in args.logs or (12, 14, 16, 18, 20, 22):
                emit(product_case(ctx, curve, log_n, reps, args.reps_host))
                emit(perm_z_case(ctx, curve, log_n, reps, args.reps_host))
                emit(quotient_case(ctx, curve, log_n, reps))
    if args.only in (None, "c"):
        for curve in args.curves:
            emit(rounds_case(ctx, curve, 20, args.reps_whole))


if __name__ == "__main__":
    main()
