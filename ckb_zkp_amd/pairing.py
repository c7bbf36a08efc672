"""Optimal-ate pairings on the MI355X backend: host-side drivers over zkp_pairing_* (include/zkp_accel.h, csrc/pairing.hip), the
counterpart of ark-ec's `PairingEngine::{miller_loop, final_exponentiation, pairing, product_of_pairings}` that the reference's
verifiers call (groth16/src/verifier.rs:8-44, marlin/src/pc/kzg10.rs:158-173).

Points are Python integers in affine form ((x, y) / ((x0, x1), (y0, y1)), None = the identity), as everywhere in this package.
A GT value is a flat list of six Fq2 pairs over the basis 1, w, ..., w^5 of Fq12 = Fq2[w] / (w^6 - xi); across the ABI it is 12
Montgomery Fq in ark's tower order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (c_j.c_i is the coefficient of w^(2 i + j)):
`fq12_to_mont` / `fq12_from_mont` convert.

Contract: `final_exponentiation(f)` is f^(k (q^12 - 1) / r) with k = GT_POWER[curve] (1 on BN254, 3 on BLS12-381; coprime to r), so
`pairing(P, Q)` is e(P, Q)^k with e the reduced pairing f^((q^12 - 1) / r): bilinear and non-degenerate; GT values are comparable
with GT values of this library only.  Nothing here tests curve or subgroup
membership (`Context.subgroup_check` does).
"""
from __future__ import annotations

import numpy as np

from . import codec
from .api import Context
from .params import get_curve

GT_POWER = {"bn254": 1, "bls12_381": 3}          # == zkp_pairing_info info[0]; csrc/pairing.hpp
# Fq products (squarings included, every Fq2 product 3 and every Fq2 squaring 2) of ONE Miller loop and ONE final exponentiation by the
# formulas of csrc/pairing_dev.hpp, counted by running them on a CPU field (tests/test_pairing_ref.py); the product tree of a group
# adds 54 per pair.  The final exponentiation's count includes its one Fq inversion (a Fermat chain of about 1.5 log2 q products).
FQ_PRODUCTS = {"bn254": dict(miller=10512, final_exp=9403), "bls12_381": dict(miller=7549, final_exp=8300)}
FQ12_MUL_PRODUCTS = 54
_FLAT_OF_ABI = [0, 2, 4, 1, 3, 5]                  # ABI position (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) -> power of w


def fq12_to_mont(f, curve) -> np.ndarray:
    """flat list of six Fq2 pairs -> (12 * fq_limbs,) uint64, the ABI's words"""
    c = get_curve(curve)
    vals = []
    for k in _FLAT_OF_ABI:
        vals += [codec._fq_mont(f[k][0], c), codec._fq_mont(f[k][1], c)]
    return codec.ints_to_limbs(vals, c.fq_limbs).reshape(-1)


def fq12_from_mont(words, curve) -> list:
    """(12 * fq_limbs,) uint64 ABI words -> flat list of six Fq2 pairs"""
    c = get_curve(curve)
    v = codec._fq_list(np.ascontiguousarray(words, dtype=np.uint64).reshape(12, c.fq_limbs), c)
    out = [None] * 6
    for pos, k in enumerate(_FLAT_OF_ABI):
        out[k] = (v[2 * pos], v[2 * pos + 1])
    return out


def gt_one() -> list:
    return [(1, 0)] + [(0, 0)] * 5


def _points(c, g1_points, g2_points):
    assert len(g1_points) == len(g2_points)
    g1, i1 = codec.g1_to_mont(list(g1_points), c)
    g2, i2 = codec.g2_to_mont(list(g2_points), c)
    return g1, i1, g2, i2


def miller_products_mont(ctx: Context, curve, g1: np.ndarray, i1: np.ndarray, g2: np.ndarray, i2: np.ndarray, group: int,
                         final_exp: bool = False) -> np.ndarray:
    """The ABI-level driver: (n, w) Montgomery points + (n,) flags -> (n / group, 12 * fq_limbs) words, one Miller product per group;
    final_exp: followed by the final exponentiation of all of them in one launch."""
    c = get_curve(curve)
    n = len(g1)
    if group < 1 or n < 1 or n % group or len(g2) != n:
        raise ValueError("n pairs form n / group groups: n >= 1, group >= 1, n a multiple of group")
    m = n // group
    out = np.zeros((m, 12 * c.fq_limbs), dtype=np.uint64)
    bufs = [ctx.to_device(a) for a in (np.ascontiguousarray(g1, dtype=np.uint64), np.ascontiguousarray(i1, dtype=np.uint8),
                                       np.ascontiguousarray(g2, dtype=np.uint64), np.ascontiguousarray(i2, dtype=np.uint8), out)]
    try:
        ctx.pairing_miller_dev(c, bufs[0], bufs[1], bufs[2], bufs[3], n, group, bufs[4])
        if final_exp:
            ctx.pairing_final_exp_dev(c, bufs[4], m, bufs[4])
        ctx.d2h(out, bufs[4])
    finally:
        for p in bufs:
            ctx.dev_free(p)
    return out


def miller_products(ctx: Context, curve, g1_points, g2_points, group: int) -> list:
    """One Fq12 per group of `group` consecutive pairs: the product of the pairs' Miller functions (defined up to factors that the
    final exponentiation removes; a pair with an identity contributes 1)."""
    c = get_curve(curve)
    return [fq12_from_mont(row, c) for row in miller_products_mont(ctx, c, *_points(c, g1_points, g2_points), group)]


def final_exponentiation(ctx: Context, curve, fs) -> list:
    """[f^(GT_POWER (q^12 - 1) / r) for f in fs] in one launch; 0 maps to 0."""
    c = get_curve(curve)
    a = np.stack([fq12_to_mont(f, c) for f in fs])
    d = ctx.to_device(a)
    try:
        ctx.pairing_final_exp_dev(c, d, len(a), d)
        ctx.d2h(a, d)
    finally:
        ctx.dev_free(d)
    return [fq12_from_mont(row, c) for row in a]


def pairing(ctx: Context, curve, p, q) -> list:
    """e(p, q)^GT_POWER for one G1 point and one G2 point."""
    return pairings(ctx, curve, [p], [q])[0]


def pairings(ctx: Context, curve, g1_points, g2_points) -> list:
    """[e(P_i, Q_i)^GT_POWER] in one launch of each kernel."""
    c = get_curve(curve)
    g1, i1, g2, i2 = _points(c, g1_points, g2_points)
    return [fq12_from_mont(row, c) for row in ctx.pairing(c, g1, i1, g2, i2)]


def product_is_one(ctx: Context, curve, g1_points, g2_points, group: int | None = None):
    """prod e(P_i, Q_i) == 1 ?  group None: one verdict over all pairs (bool).  Otherwise a list of n / group verdicts, one per group
    of consecutive pairs, from one Miller launch and one final exponentiation launch."""
    c = get_curve(curve)
    g1, i1, g2, i2 = _points(c, g1_points, g2_points)
    n = len(g1)
    g = n if group is None else group
    if g < 1 or n < 1 or n % g:
        raise ValueError("n pairs form n / group groups: n >= 1, group >= 1, n a multiple of group")
    ok = ctx.pairing_check(c, g1, i1, g2, i2, g)
    return bool(ok[0]) if group is None else [bool(x) for x in ok]
