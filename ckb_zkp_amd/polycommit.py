"""Matrix polynomial commitments of hyrax, libra and spartan on the device, function by function against the reference:
`poly_commit_vec` / `packing_poly_commit` (spartan/src/commitments.rs:10-56, libra/src/evaluate.rs:130-170) and
LogDotProductProof::prover / ::reduce_prover over BulletReduceProof::prover (hyrax/src/commitment.rs:335-578, the same text in
libra/src/commitment.rs).

  * every commitment over gen_n goes through the resident key (zkp_pedersen_commit_rows_dev): l_size rows in three launches;
  * reduce_prover: two zkp_fr_eq_evals_dev tables, lz = L^T M by zkp_fr_vecmat_dev over the device-resident polynomial,
    lz_blind = <L, blinds> by zkp_fr_dot_batch_dev, then log_dot_product_prove;
  * log_dot_product_prove: comm_x from the key, comm_y / delta / beta as small batched MSMs (zkp_msm_g1_var_batch_dev), the
    reduction is ipa.inner_product_prove unchanged (BulletReduceProof::prover is called with (x_vec, a_vec); its (a, b) come back
    as (x_hat, a_hat)).

Points are (xy, inf) — affine Montgomery limbs and an identity flag — and scalars Python integers.  `rand` is a callable or a
sequence of exactly the values the prover draws (bulletproofs.drawer), in the reference's order.  The merlin transcript stays with
the caller: `challenger.append(label, point)` and `challenger.challenge(label) -> int` are called in the reference's order with the
reference's labels: Cx, Cy, then L, R -> x per round, then delta, beta -> c.

Out of scope: DotProductProof (linear size), EqProof / KnowledgeProof / ProductProof (a handful of scalar multiplications), G2, the
verifiers (tests/polycommit_ref.py has them in Python integers), whole Hyrax / Libra / Spartan provers."""
from __future__ import annotations

import random
import time

import numpy as np

from . import codec
from .bulletproofs import drawer
from .ipa import inner_product_prove
from .params import get_curve

PEDERSEN_MAX_GENS = 1 << 16         # ZKP_PEDERSEN_MAX_GENS
VECMAT_ROW_CHUNK = 32               # ZKP_FR_VECMAT_ROW_CHUNK
PEDERSEN_ROW_LANES = 64             # csrc/pedersen.hpp PED_LANES: lane t of the row pass adds slices t, t + 64, ... of its row
MAX_CELLS = 1 << 28                 # rows * cols of one zkp_pedersen_commit_rows_dev / zkp_fr_vecmat_dev call


def split_sizes(num_vars: int):
    """(l_size, r_size) of a polynomial in num_vars variables: 2^floor(s / 2) rows of 2^(s - floor(s / 2)) evaluations"""
    return 1 << (num_vars // 2), 1 << (num_vars - num_vars // 2)


def _log2(n: int) -> int:
    assert n >= 1 and n & (n - 1) == 0, "a power of two"
    return n.bit_length() - 1


class Params:
    """PolyCommitmentSetupParameters: gen_n (n generators and h) with its device key, gen_1 (one generator g1; gen_1.h is gen_n.h)"""

    def __init__(self, ctx, curve, gens_xy, gens_inf, h_xy, g1_xy):
        self.ctx, self.curve = ctx, get_curve(curve)
        self.gens_xy = np.ascontiguousarray(gens_xy, dtype=np.uint64)
        self.n = self.gens_xy.shape[0]
        self.gens_inf = np.zeros(self.n, dtype=np.uint8) if gens_inf is None else np.ascontiguousarray(gens_inf, dtype=np.uint8)
        self.h_xy = np.ascontiguousarray(h_xy, dtype=np.uint64).reshape(-1)
        self.g1_xy = np.ascontiguousarray(g1_xy, dtype=np.uint64).reshape(-1)
        self.key = ctx.pedersen_key_create(self.curve, self.gens_xy, self.gens_inf, self.h_xy)

    def free(self):
        if self.key:
            self.ctx.pedersen_key_free(self.key)
            self.key = None


def setup(ctx, curve, num_vars: int, seed) -> Params:
    """generators for polynomials of num_vars variables: seeded multiples of the group generator (zkp_fixed_base_mul_g1)"""
    c = get_curve(curve)
    n = split_sizes(num_vars)[1]
    rng = random.Random(seed)
    base = codec.g1_to_mont([c.g1], c)[0][0]
    xy, inf = ctx.fixed_base_mul(c, 1, base, codec.fr_canonical([rng.randrange(1, c.r) for _ in range(n + 2)], c))
    return Params(ctx, c, xy[:n], inf[:n], xy[n], xy[n + 1])


class DevicePoly:
    """the evaluations of a polynomial resident on the device (Montgomery Fr): commit and open without a second upload"""

    def __init__(self, ctx, curve, values):
        """values: integers, or an (n, 4) array of Montgomery words"""
        self.ctx, self.n = ctx, len(values)
        words = values if isinstance(values, np.ndarray) else codec.fr_to_mont(values, get_curve(curve))
        self.ptr = ctx.to_device(np.ascontiguousarray(words, dtype=np.uint64))

    def free(self):
        if self.ptr:
            self.ctx.dev_free(self.ptr)
            self.ptr = None


def _commit_rows(params: Params, values, rows: int, cols: int, blinds):
    """values: rows * cols integers, a (rows * cols, 4) Montgomery array or a DevicePoly; blinds: rows integers or None"""
    ctx, c = params.ctx, params.curve
    w = 2 * c.fq_limbs
    bufs = []

    def up(arr):
        d = ctx.to_device(arr)
        bufs.append(d)
        return d

    try:
        if isinstance(values, DevicePoly):
            ds = values.ptr
        else:
            ds = up(values if isinstance(values, np.ndarray) else codec.fr_to_mont(values, c))
        db = None if blinds is None else up(codec.fr_to_mont(blinds, c))
        xy, inf = np.zeros((rows, w), dtype=np.uint64), np.zeros(rows, dtype=np.uint8)
        dxy, dinf = up(xy), up(inf)
        ctx.pedersen_commit_rows_dev(params.key, ds, rows, cols, db, dxy, dinf)
        ctx.d2h(xy, dxy)
        ctx.d2h(inf, dinf)
        return [(xy[i], bool(inf[i])) for i in range(rows)]
    finally:
        for p in bufs:
            ctx.dev_free(p)


def poly_commit_vec(params: Params, values, blind: int):
    """sum_j values[j] g_j + blind h over gen_n -> (xy, inf)"""
    n = values.shape[0] if isinstance(values, np.ndarray) else len(values)
    assert 1 <= n <= params.n
    return _commit_rows(params, values, 1, n, [blind])[0]


def packing_poly_commit(params: Params, values, rand, is_blind: bool):
    """one commitment per row of the l_size x r_size matrix of evaluations -> (commits, blinds): one blind per row, drawn in row
    order; zero without is_blind"""
    n = values.n if isinstance(values, DevicePoly) else len(values)
    l_size, r_size = split_sizes(_log2(n))
    assert r_size <= params.n
    blinds = drawer(rand, l_size)(l_size) if is_blind else [0] * l_size
    blinds = [b % params.curve.r for b in blinds]
    return _commit_rows(params, values, l_size, r_size, blinds if is_blind else None), blinds


def _small_msms(params: Params, entries):
    """entries: lists of (scalar, (xy, inf)) -> one affine point each, in ONE zkp_msm_g1_var_batch_dev call"""
    ctx, c = params.ctx, params.curve
    xys = [np.stack([np.asarray(p[0], dtype=np.uint64) for _, p in e]) for e in entries]
    infs = [np.array([1 if p[1] else 0 for _, p in e], dtype=np.uint8) for e in entries]
    scalars = [codec.fr_to_mont([s for s, _ in e], c) for e in entries]
    jac = ctx.msm_var_batch(c, 1, xys, infs, scalars, montgomery=True)
    return [ctx.into_affine(c, 1, j) for j in jac]


def log_dot_product_prove(params: Params, x_vec, blind_x: int, a_vec, y: int, blind_y: int, rand, challenger, stats: dict | None = None):
    """LogDotProductProof::prover: <x_vec, a_vec> = y under comm_x and comm_y.  x_vec, a_vec: integers or (n, 4) Montgomery arrays.
    Returns (proof, comm_x, comm_y), proof = (l_vec, r_vec, delta, beta, z1, z2)."""
    ctx, c = params.ctx, params.curve
    r = c.r
    xm = x_vec if isinstance(x_vec, np.ndarray) else codec.fr_to_mont(x_vec, c)
    am = a_vec if isinstance(a_vec, np.ndarray) else codec.fr_to_mont(a_vec, c)
    size = xm.shape[0]
    assert am.shape[0] == size and params.n >= size
    k = _log2(size)
    draw = drawer(rand, 3 + 2 * k)
    d, r_beta, r_delta = (v % r for v in draw(3))
    blind_vec = [tuple(v % r for v in draw(2)) for _ in range(k)]
    h, g1 = (params.h_xy, False), (params.g1_xy, False)
    t0 = time.perf_counter()

    comm_x = poly_commit_vec(params, xm, blind_x)
    challenger.append("Cx", comm_x)
    comm_y = _small_msms(params, [[(y, g1), (blind_y, h)]])[0]
    challenger.append("Cy", comm_y)
    t1 = time.perf_counter()

    def challenge(l_xy, l_inf, r_xy, r_inf):
        challenger.append("L", (l_xy, l_inf))
        challenger.append("R", (r_xy, r_inf))
        return challenger.challenge("x")

    l_vec, r_vec, x_hat, a_hat, g_hat, r_hat_gamma = inner_product_prove(
        ctx, c, params.gens_xy[:size], params.gens_inf[:size], params.g1_xy, params.h_xy, xm, am,
        codec.fr_mont((blind_x + blind_y) % r, c), [(codec.fr_mont(bl, c), codec.fr_mont(br, c)) for bl, br in blind_vec], challenge)
    x_hat, a_hat, r_hat_gamma = codec.fr_int(x_hat, c), codec.fr_int(a_hat, c), codec.fr_int(r_hat_gamma, c)
    y_hat = x_hat * a_hat % r
    t2 = time.perf_counter()

    delta, beta = _small_msms(params, [[(d, g_hat), (r_delta, h)], [(d, g1), (r_beta, h)]])
    challenger.append("delta", delta)
    challenger.append("beta", beta)
    ch = challenger.challenge("c") % r
    z1 = (d + ch * y_hat) % r
    z2 = (a_hat * (ch * r_hat_gamma + r_beta) + r_delta) % r
    if stats is not None:
        t3 = time.perf_counter()
        stats.update(ms_commit_xy=1e3 * (t1 - t0), ms_reduce=1e3 * (t2 - t1), ms_tail=1e3 * (t3 - t2))
    return (l_vec, r_vec, delta, beta, z1, z2), comm_x, comm_y


def reduce_prover(params: Params, poly, blind_poly, ry, ry_blind: int, eval_: int, rand, challenger, stats: dict | None = None):
    """LogDotProductProof::reduce_prover: opens the committed polynomial (integers or a DevicePoly) at rx ++ ry = `ry` to `eval_`.
    blind_poly: the l_size blinds of packing_poly_commit, or [] for none.  Returns (proof, comm_y)."""
    ctx, c = params.ctx, params.curve
    n = poly.n if isinstance(poly, DevicePoly) else len(poly)
    size = _log2(n)
    assert len(ry) == size
    l_size, r_size = split_sizes(size)
    blinds = list(blind_poly) if len(blind_poly) else [0] * l_size
    assert len(blinds) == l_size and l_size * r_size <= MAX_CELLS
    own = None if isinstance(poly, DevicePoly) else DevicePoly(ctx, c, poly)
    bufs = []
    t0 = time.perf_counter()
    try:
        dl, dr, dlz = (ctx.dev_alloc(32 * m) for m in (l_size, r_size, r_size))
        bufs += [dl, dr, dlz]
        db = ctx.to_device(codec.fr_to_mont(blinds, c))
        bufs.append(db)
        ctx.fr_eq_evals_dev(c, codec.fr_to_mont(ry[:size // 2], c), dl)
        ctx.fr_eq_evals_dev(c, codec.fr_to_mont(ry[size // 2:], c), dr)
        ctx.sync()
        t1 = time.perf_counter()
        ctx.fr_vecmat_dev(c, dl, (own or poly).ptr, l_size, r_size, dlz)
        lz_blind = codec.fr_int(ctx.fr_dot_batch_dev(c, [dl], [db], [l_size])[0], c)
        lz, r_eq = np.zeros((r_size, 4), dtype=np.uint64), np.zeros((r_size, 4), dtype=np.uint64)
        ctx.d2h(lz, dlz)
        ctx.d2h(r_eq, dr)
        t2 = time.perf_counter()
    finally:
        for p in bufs:
            ctx.dev_free(p)
        if own is not None:
            own.free()
    if stats is not None:
        stats.update(ms_eq_tables=1e3 * (t1 - t0), ms_row_fold=1e3 * (t2 - t1))
    proof, _, comm_y = log_dot_product_prove(params, lz, lz_blind, r_eq, eval_, ry_blind, rand, challenger, stats)
    return proof, comm_y
