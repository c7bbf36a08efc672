#!/usr/bin/env python3
"""The Fr hot path of the Bulletproofs R1CS prover on the device.  HIP events around each alternative (zkp_timer_*), warm-up 3, the
median of --reps (>= 20); the alternatives of a comparison take turns inside one loop of one process; both are checked to give
the same words in the same run.  One JSON line per case.  n = n_w = n_s = N.
  (a) zkp_fr_bp_t_coeffs_dev against its composition from the exports that existed before it: eight zkp_fr_vec_op_dev launches
      build l2, r0, r1, r2, r5 over vectors padded to N, one zkp_fr_dot_batch_dev of sixteen entries multiplies them, the host adds
      the sixteen products into t2 .. t10.  The composition takes y^i, y^-i and z^(i+1) uploaded from the host: that time is
      reported apart (powers_upload_ms).
  (b) zkp_fr_bp_lr_eval_dev against the same eight launches, two zkp_fr_lincomb_dev calls for l(x) and r(x) and one
      zkp_fr_dot_batch_dev for t_x.
      Both against the library's copy kernel (zkp_bench_hbm_copy) over the bytes they must move: 7 N elements read, and 2 N written
      by (b).
  (c) one a / b round of the inner-product argument through zkp_fr_ipa_fold_ab_dev against four zkp_fr_vec_op_dev launches and one
      zkp_fr_dot_batch_dev call of two entries (six launches).
  (d) a whole bulletproofs.prove split by stage (host wall time, driver included).

    python tools/bulletproofs_bench.py [--reps 20] [--quick] [--only a|c|d] [--logs 10 16 20]
--quick: one call of every kind at N = 2^10 and nothing else (for a kernel trace that counts launches).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import bulletproofs, codec  # noqa: E402
from ckb_zkp_amd.api import VEC_ADD, VEC_AXPY, VEC_MUL, VEC_SCALE, VEC_SUB, Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402
from ckb_zkp_amd.r1cs import R1csInstance  # noqa: E402

# (l index, r index) of the sixteen products and the t they belong to (VecPoly5::special_inner_product)
PRODUCTS = [(2, 0, 2), (2, 1, 3), (3, 0, 3), (2, 2, 4), (3, 1, 4), (4, 0, 4), (3, 2, 5), (4, 1, 5), (5, 0, 5), (4, 2, 6), (5, 1, 6),
            (2, 5, 7), (5, 2, 7), (3, 5, 8), (4, 5, 9), (5, 5, 10)]


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


def rand_fr(rng, c, n):
    """n reduced values as Montgomery words (any words below r are a valid vector for timing)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


class Composed:
    """l(X), r(X) from zkp_fr_vec_op_dev / zkp_fr_dot_batch_dev / zkp_fr_lincomb_dev over vectors of N elements"""

    def __init__(self, ctx, c, d_in, N, y, z):
        self.ctx, self.c, self.N = ctx, c, N
        self.aL, self.aR, self.aO, self.w, self.v, self.sL, self.sR = d_in
        r = c.r
        self.zn = pow(z, N, r)
        yi = pow(y, -1, r)
        ys, yis, zs, a, b, e = [], [], [], 1, 1, z
        for _ in range(N):
            ys.append(a)
            yis.append(b)
            zs.append(e)
            a, b, e = a * y % r, b * yi % r, e * z % r
        host = [codec.fr_to_mont(t, c) for t in (ys, yis, zs)]
        ctx.timer_start()
        self.d_y, self.d_yi, self.d_z = (ctx.to_device(h) for h in host)
        self.upload_ms = ctx.timer_stop_ms()
        self.tmp = [ctx.dev_alloc(32 * N) for _ in range(8)]       # l2, r0, r1, r2, r5, scratch, l_x, r_x
        self.launches = 0

    def coefficients(self):
        ctx, c, N, r = self.ctx, self.c, self.N, self.c.r
        l2, r0, r1, r2, r5, t = self.tmp[:6]
        m = lambda v: codec.fr_mont(v % r, c)                     # noqa: E731
        ctx.fr_vec_op(c, VEC_MUL, self.d_yi, self.d_z, t, N)                       # U = zn Z / Y
        ctx.fr_vec_op(c, VEC_AXPY, self.aL, t, l2, N, m(self.zn))                  # l2 = aL + U
        ctx.fr_vec_op(c, VEC_SCALE, self.v, None, r0, N, m(-1))                    # r0 = -v
        ctx.fr_vec_op(c, VEC_SCALE, self.d_z, None, t, N, m(self.zn * self.zn))    # r1 = zn^2 Z - Y
        ctx.fr_vec_op(c, VEC_SUB, t, self.d_y, r1, N)
        ctx.fr_vec_op(c, VEC_MUL, self.d_y, self.aR, t, N)                         # r2 = Y aR + Z
        ctx.fr_vec_op(c, VEC_ADD, t, self.d_z, r2, N)
        ctx.fr_vec_op(c, VEC_MUL, self.d_y, self.sR, r5, N)                        # r5 = Y sR
        return {2: l2, 3: self.aO, 4: self.w, 5: self.sL}, {0: r0, 1: r1, 2: r2, 5: r5}

    def t_products(self):
        lp, rp = self.coefficients()
        return self.ctx.fr_dot_batch_dev(self.c, [lp[a] for a, _, _ in PRODUCTS], [rp[b] for _, b, _ in PRODUCTS], [self.N] * len(PRODUCTS))

    def t_coeffs(self):
        """t2 .. t10 as integers"""
        c = self.c
        t = {d: 0 for d in range(2, 11)}
        for (_, _, d), e in zip(PRODUCTS, self.t_products()):
            t[d] = (t[d] + codec.fr_int(e, c)) % c.r
        return [t[d] for d in range(2, 11)]

    def lr_eval(self, x):
        ctx, c, N, r = self.ctx, self.c, self.N, self.c.r
        lp, rp = self.coefficients()
        l_x, r_x = self.tmp[6:8]
        ctx.fr_lincomb_dev(c, [lp[d] for d in (2, 3, 4, 5)], [N] * 4, codec.fr_to_mont([pow(x, d, r) for d in (2, 3, 4, 5)], c), l_x, N)
        ctx.fr_lincomb_dev(c, [rp[d] for d in (0, 1, 2, 5)], [N] * 4, codec.fr_to_mont([pow(x, d, r) for d in (0, 1, 2, 5)], c), r_x, N)
        return ctx.fr_dot_batch_dev(c, [l_x], [r_x], [N])[0]

    def free(self):
        for p in [self.d_y, self.d_yi, self.d_z] + self.tmp:
            self.ctx.dev_free(p)


def read(ctx, ptr, n):
    a = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(a, ptr)
    return a


def lr_case(ctx, curve, log_n, reps):
    c = get_curve(curve)
    r = c.r
    N = 1 << log_n
    rng = np.random.default_rng(log_n)
    d_in = [ctx.to_device(rand_fr(rng, c, N)) for _ in range(7)]
    d_lx, d_rx = ctx.dev_alloc(32 * N), ctx.dev_alloc(32 * N)
    y, z, x = (int.from_bytes(rng.bytes(31), "little") for _ in range(3))
    ym, zm, xm = (codec.fr_mont(v, c) for v in (y, z, x))
    vecs = ctx.bp_vectors(*d_in, N, N, N, N)
    comp = Composed(ctx, c, d_in, N, y, z)
    try:
        t_fused = [codec.fr_int(e, c) for e in ctx.fr_bp_t_coeffs_dev(c, vecs, ym, zm)]
        same_t = t_fused == comp.t_coeffs()
        tx_fused = ctx.fr_bp_lr_eval_dev(c, vecs, ym, zm, xm, d_lx, d_rx)
        tx_comp = comp.lr_eval(x)
        same_lr = bool(np.array_equal(tx_fused, tx_comp) and np.array_equal(read(ctx, d_lx, N), read(ctx, comp.tmp[6], N))
                       and np.array_equal(read(ctx, d_rx, N), read(ctx, comp.tmp[7], N)))
        fns = {"t_fused": lambda: ctx.fr_bp_t_coeffs_dev(c, vecs, ym, zm), "t_composed": comp.t_products,
               "t_composed_again": comp.t_products,                # the composition against itself: the spread between two runs
               "lr_fused": lambda: ctx.fr_bp_lr_eval_dev(c, vecs, ym, zm, xm, d_lx, d_rx), "lr_composed": lambda: comp.lr_eval(x),
               "lr_composed_again": lambda: comp.lr_eval(x)}
        t = timed_alternating(ctx, fns, reps)
        gbs = ctx.bench_hbm_copy(max(32 * 7 * N, 1 << 20))
        floor_t, floor_lr = 32 * 7 * N / (gbs * 1e9) * 1e3, 32 * 9 * N / (gbs * 1e9) * 1e3
        line = dict(case="lr", curve=curve, log_n=log_n, same_t=same_t, same_lr=same_lr, powers_upload_ms=round(comp.upload_ms, 4),
                    launches=dict(t_fused=2, t_composed=10, lr_fused=2, lr_composed=12), copy_gb_per_s=round(gbs, 1),
                    copy_floor_t_ms=round(floor_t, 5), copy_floor_lr_ms=round(floor_lr, 5))
        for k, (med, mn) in t.items():
            line[k + "_ms"], line[k + "_min_ms"] = round(med, 4), round(mn, 4)
        line.update(t_composed_over_fused=round(t["t_composed"][0] / t["t_fused"][0], 2),
                    lr_composed_over_fused=round(t["lr_composed"][0] / t["lr_fused"][0], 2),
                    t_fused_over_floor=round(t["t_fused"][0] / floor_t, 1), lr_fused_over_floor=round(t["lr_fused"][0] / floor_lr, 1))
        return [line]
    finally:
        ctx.sync()
        comp.free()
        for p in d_in + [d_lx, d_rx]:
            ctx.dev_free(p)


def fold_composed(ctx, c, pa, pb, n, xm, xim):
    m = n // 2
    h = m // 2
    ctx.fr_vec_op(c, VEC_SCALE, pa, None, pa, m, xm)
    ctx.fr_vec_op(c, VEC_AXPY, pa, pa + 32 * m, pa, m, xim)
    ctx.fr_vec_op(c, VEC_SCALE, pb, None, pb, m, xim)
    ctx.fr_vec_op(c, VEC_AXPY, pb, pb + 32 * m, pb, m, xm)
    return ctx.fr_dot_batch_dev(c, [pa, pa + 32 * h], [pb + 32 * h, pb], [h, h])


def fold_case(ctx, curve, log_n, reps):
    c = get_curve(curve)
    n = 1 << log_n
    rng = np.random.default_rng(50 + log_n)
    host = rand_fr(rng, c, 2 * n)
    d_f, d_c = ctx.to_device(host), ctx.to_device(host)
    x = int.from_bytes(rng.bytes(31), "little") | 1
    xm, xim = codec.fr_mont(x, c), codec.fr_mont(pow(x, -1, c.r), c)
    try:
        cs_f = ctx.fr_ipa_fold_ab_dev(c, d_f, d_f + 32 * n, n, xm)
        cs_c = fold_composed(ctx, c, d_c, d_c + 32 * n, n, xm, xim)
        same = bool(np.array_equal(cs_f, cs_c) and np.array_equal(read(ctx, d_f, 2 * n), read(ctx, d_c, 2 * n)))
        fns = {"fused": lambda: ctx.fr_ipa_fold_ab_dev(c, d_f, d_f + 32 * n, n, xm),       # in place again and again: the time does not
               "composed": lambda: fold_composed(ctx, c, d_c, d_c + 32 * n, n, xm, xim),   # depend on the values
               "composed_again": lambda: fold_composed(ctx, c, d_c, d_c + 32 * n, n, xm, xim)}
        t = timed_alternating(ctx, fns, reps)
        line = dict(case="fold_ab", curve=curve, log_n=log_n, same_words=same, launches=dict(fused=2, composed=6))
        for k, (med, mn) in t.items():
            line[k + "_ms"], line[k + "_min_ms"] = round(med, 4), round(mn, 4)
        line["composed_over_fused"] = round(t["composed"][0] / t["fused"][0], 2)
        return [line]
    finally:
        ctx.sync()
        ctx.dev_free(d_f)
        ctx.dev_free(d_c)


class HashChallenger:
    def __init__(self, c):
        self.r, self.state = c.r, b"bench"

    def _next(self, data):
        self.state = hashlib.sha256(self.state + data).digest()
        return int.from_bytes(self.state, "little") % self.r or 1

    def yz(self, *pts):
        return self._next(b"".join(p[0].tobytes() for p in pts)), self._next(b"z")

    def x(self, pts):
        return self._next(b"".join(p[0].tobytes() for p in pts))

    def x1(self, t_x, tau_x, mu, l_x, r_x):
        return self._next(int(t_x).to_bytes(32, "little") + l_x[:4].tobytes() + r_x[:4].tobytes())

    def ipa(self, l_pt, r_pt):
        return self._next(l_pt[0].tobytes() + r_pt[0].tobytes())


def whole_case(ctx, curve, log_n, reps):
    """n = N constraints of two terms per row over N / 2 aux variables (the prover does not need a satisfied system)"""
    c = get_curve(curve)
    N = 1 << log_n
    n_w, k = N // 2, 2
    rng = np.random.default_rng(70 + log_n)

    def csr():
        return (np.arange(0, 2 * N + 1, 2, dtype=np.uint32), rng.integers(0, k + n_w, size=2 * N, dtype=np.uint32), rand_fr(rng, c, 2 * N))

    r1cs = R1csInstance(c, k, n_w, N, csr(), csr(), csr(), z=[1] + codec.fr_from_mont(rand_fr(rng, c, k + n_w - 1), c))
    gen_xy, _ = codec.g1_to_mont([c.g1], c)
    pts, inf = ctx.fixed_base_mul(c, 1, gen_xy[0], codec.fr_canonical(codec.fr_from_mont(rand_fr(rng, c, 2 * N + 3), c), c))
    assert not inf.any()
    gens = bulletproofs.Generators(pts[:N], pts[N:2 * N], pts[2 * N], pts[2 * N + 1], pts[2 * N + 2])
    rand = codec.fr_from_mont(rand_fr(rng, c, 2 * N + 12), c)
    runs = []
    for _ in range(reps + 1):
        stats = {}
        ctx.timer_start()
        bulletproofs.prove(ctx, c, r1cs, gens, rand, HashChallenger(c), stats=stats)
        stats["total_ms"] = ctx.timer_stop_ms()
        runs.append(stats)
    runs = runs[1:]                                                # the first run is the warm-up
    med = lambda key: float(np.median([s[key] for s in runs]))    # noqa: E731
    stages = ("upload", "commit_a", "v", "t", "lr", "ipp_p", "ipa")
    return [dict(case="prove", curve=curve, log_n=log_n, n=N, n_w=n_w, reps=reps, total_ms=round(med("total_ms"), 2),
                 **{s + "_ms": round(1e3 * med(s), 2) for s in stages},
                 note="host wall time per stage (every call returns when its work is done), host driver and conversions included")]


def quick(ctx):
    """one call of every kind, no warm-up, so that a kernel trace shows the launches per call"""
    c = get_curve("bn254")
    N = 1 << 10
    rng = np.random.default_rng(1)
    d_in = [ctx.to_device(rand_fr(rng, c, N)) for _ in range(7)]
    d_lx, d_rx = ctx.dev_alloc(32 * N), ctx.dev_alloc(32 * N)
    m = codec.fr_mont(77, c)
    vecs = ctx.bp_vectors(*d_in, N, N, N, N)
    ctx.fr_powers_dev(c, m, m, d_lx, N)
    ctx.fr_bp_t_coeffs_dev(c, vecs, m, m)
    ctx.fr_bp_lr_eval_dev(c, vecs, m, m, m, d_lx, d_rx)
    ctx.fr_ipa_fold_ab_dev(c, d_lx, d_rx, N, m)
    ctx.fr_ipa_fold_ab_dev(c, d_lx, d_rx, N, m, want_c=False)
    ctx.sync()
    for p in d_in + [d_lx, d_rx]:
        ctx.dev_free(p)
    print(json.dumps(dict(case="quick", log_n=10,
                          calls=["powers: 1 launch", "t_coeffs: 2 launches", "lr_eval: 2 launches", "fold_ab with cL, cR: 2 launches",
                                 "fold_ab without: 1 launch"],
                          expected_kernel_calls=dict(powers_kernel=1, t_coeffs_kernel=1, lr_eval_kernel=1, fold_ab_kernel=2, fr_sum_partials_kernel=3))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-whole", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="one call of every kind at N = 2^10 (for a kernel trace)")
    ap.add_argument("--only", choices=["a", "c", "d"], default=None, help="a: (a) and (b)")
    ap.add_argument("--logs", type=int, nargs="*", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    if args.quick:
        return quick(ctx)
    reps = max(args.reps, 20)
    emit = lambda lines: [print(json.dumps(line), flush=True) for line in lines]    # noqa: E731
    logs = args.logs or (10, 16, 20)
    if args.only in (None, "a"):
        for lg in logs:
            emit(lr_case(ctx, "bn254", lg, reps))
        emit(lr_case(ctx, "bls12_381", 16, reps))
    if args.only in (None, "c"):
        for lg in logs:
            emit(fold_case(ctx, "bn254", lg, reps))
        emit(fold_case(ctx, "bls12_381", 16, reps))
    if args.only in (None, "d"):
        for lg in [v for v in logs if v <= 16]:
            emit(whole_case(ctx, "bn254", lg, args.reps_whole))


if __name__ == "__main__":
    main()
