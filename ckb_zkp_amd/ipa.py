"""Inner-product argument prover on the device: `bullet_inner_product_proof` (spartan/src/inner_product.rs:12-100; the same rounds as
hyrax/src/commitment.rs:491-575) over G1, with the generators, a and b resident on the device from upload to the last round.

Per round (n -> n / 2):
  * cl = <al, br>, cr = <ar, bl>: one zkp_fr_dot_batch_dev call (count 2);
  * L = <al, gr> + cl q + blind_l h, R = <ar, gl> + cr q + blind_r h: one zkp_msm_g1_var_batch_dev call with 4 entries, the pairs
    added with Context.fold and made affine with Context.into_affine.  A round whose half length exceeds ZKP_MSM_SMALL_MAX_G1
    copies that round's halves to the host and runs zkp_msm_g1_var instead;
  * x = challenge(L, R) (the merlin transcript of the reference is the caller's: any function of L and R to a non-zero Fr);
  * g_new = x^-1 gl + x gr in place over the low half (zkp_g1_ipa_fold_dev);
  * a_new = x al + x^-1 ar, b_new = x^-1 bl + x br (zkp_fr_vec_op_dev SCALE then AXPY, in place over the low halves);
  * blind_fin += x^2 blind_l + x^-2 blind_r (host).
Fr scalars in and out are Montgomery (4 x u64), points affine Montgomery with identity flags, as elsewhere in the library."""
from __future__ import annotations

import numpy as np

from .api import VEC_AXPY, VEC_SCALE
from .codec import fr_int, fr_mont
from .params import get_curve

MSM_SMALL_MAX_G1 = 1 << 16          # ZKP_MSM_SMALL_MAX_G1


def inner_product_prove(ctx, curve, g_xy, g_inf, q_xy, h_xy, a, b, gamma_blind, blinds, challenge):
    """g_xy: (n, w) affine Montgomery generators (n a power of two), g_inf: (n,) flags or None; q_xy, h_xy: one point each;
    a, b: (n, 4) Montgomery Fr; gamma_blind: Montgomery Fr; blinds: log2(n) pairs (blind_l, blind_r) of Montgomery Fr;
    challenge(l_xy, l_inf, r_xy, r_inf) -> int.
    Returns (l_vec, r_vec, a, b, g, blind_fin): l_vec / r_vec lists of (xy, inf) affine points, a / b / blind_fin Montgomery Fr,
    g = (xy, inf) — the tuple of the reference's Ok(...), the proof's two vectors first."""
    c = get_curve(curve)
    r = c.r
    g_xy = np.ascontiguousarray(g_xy, dtype=np.uint64)
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    n = g_xy.shape[0]
    assert n >= 1 and n & (n - 1) == 0 and a.shape[0] == n and b.shape[0] == n
    assert len(blinds) >= n.bit_length() - 1
    w = g_xy.shape[1]
    ab = 8 * w
    g_flags = np.zeros(n, dtype=np.uint8) if g_inf is None else np.ascontiguousarray(g_inf, dtype=np.uint8)[:n].copy()
    qh = np.ascontiguousarray(np.stack([np.asarray(q_xy, dtype=np.uint64).reshape(w), np.asarray(h_xy, dtype=np.uint64).reshape(w)]))
    bufs = []

    def up(arr):
        d = ctx.to_device(arr)
        bufs.append(d)
        return d

    try:
        dg, dgi, da, db, dqh = up(g_xy), up(g_flags), up(a), up(b), up(qh)
        ds = up(np.zeros((4, 4), dtype=np.uint64))            # [cl, blind_l, cr, blind_r] of the round
        blind_fin = fr_int(gamma_blind, c)
        l_vec, r_vec = [], []
        rnd = 0
        while n > 1:
            n //= 2
            al, ar, bl, br = da, da + 32 * n, db, db + 32 * n
            gl, gr, gli, gri = dg, dg + ab * n, dgi, dgi + n
            cl, cr = ctx.fr_dot_batch_dev(c, [al, ar], [br, bl], [n, n])
            bl_, br_ = blinds[rnd]
            rnd += 1
            ctx.h2d(ds, np.stack([cl, np.asarray(bl_, dtype=np.uint64), cr, np.asarray(br_, dtype=np.uint64)]))
            if n <= MSM_SMALL_MAX_G1:
                jac = ctx.msm_var_batch_dev(c, 1, [gr, gl, dqh, dqh], [gri, gli, None, None], [al, ar, ds, ds + 64], [n, n, 2, 2],
                                            montgomery=True)
            else:                                             # above the batch cap: this round's halves through the host
                def host(ptr, shape, dtype):
                    h = np.zeros(shape, dtype=dtype)
                    ctx.d2h(h, ptr)
                    return h
                gxy = host(dg, (2 * n, w), np.uint64)
                gf = host(dgi, (2 * n,), np.uint8)
                av = host(da, (2 * n, 4), np.uint64)
                small = ctx.msm_var_batch_dev(c, 1, [dqh, dqh], None, [ds, ds + 64], [2, 2], montgomery=True)
                jac = np.stack([ctx.msm_var(c, 1, gxy[n:], gf[n:], av[:n], montgomery=True),
                                ctx.msm_var(c, 1, gxy[:n], gf[:n], av[n:], montgomery=True), small[0], small[1]])
            l_xy, l_inf = ctx.into_affine(c, 1, ctx.fold(c, 1, np.concatenate([jac[0], jac[2]])))
            r_xy, r_inf = ctx.into_affine(c, 1, ctx.fold(c, 1, np.concatenate([jac[1], jac[3]])))
            l_vec.append((l_xy, l_inf))
            r_vec.append((r_xy, r_inf))
            x = challenge(l_xy, l_inf, r_xy, r_inf) % r
            assert x != 0
            xi = pow(x, -1, r)
            xm, xim = fr_mont(x, c), fr_mont(xi, c)
            ctx.ipa_fold_dev(c, gl, gli, gr, gri, n, xim, xm, gl, gli)
            ctx.fr_vec_op(c, VEC_SCALE, al, None, al, n, xm)         # a' = x al + x^-1 ar
            ctx.fr_vec_op(c, VEC_AXPY, al, ar, al, n, xim)
            ctx.fr_vec_op(c, VEC_SCALE, bl, None, bl, n, xim)        # b' = x^-1 bl + x br
            ctx.fr_vec_op(c, VEC_AXPY, bl, br, bl, n, xm)
            blind_fin = (blind_fin + x * x * fr_int(bl_, c) + xi * xi * fr_int(br_, c)) % r
        a_fin, b_fin = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        g_fin, g_fin_inf = np.zeros(w, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
        ctx.d2h(a_fin, da)
        ctx.d2h(b_fin, db)
        ctx.d2h(g_fin, dg)
        ctx.d2h(g_fin_inf, dgi)
        return l_vec, r_vec, a_fin, b_fin, (g_fin, bool(g_fin_inf[0])), fr_mont(blind_fin, c)
    finally:
        for p in bufs:
            ctx.dev_free(p)
