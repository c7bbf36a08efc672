"""aSVC subvector commitments on the device (asvc/src/lib.rs), function by function: key_gen (:76-158), commit (:160-180),
prove_pos (:182-225), update_commit (:339-363), update_proof (:365-403), aggregate_proofs (:405-439), and the batched forms
update_commit_many / update_proof_many.

  * key_gen: the 3 n exponents d_i = 1 / (tau - w^i), a_i = (tau^n - 1) d_i, l_i = a_i w^i / n, u_i = (l_i - 1) d_i are formed on the
    device from zkp_fr_powers_dev, zkp_fr_vec_op_dev and zkp_fr_batch_inverse_dev and leave it as canonical words (a ZKP_VEC_SCALE by
    the raw word 1 is a Montgomery product by R^-1, ark's into_repr()); the points are zkp_fixed_base_mul_g1 / _g2 calls;
  * commit: the values go to the device once, then zkp_msm_g1_mont_dev over the resident l_of_g1;
  * prove_pos: zkp_ntt_dev (inverse), zkp_fr_asvc_quotient_dev, zkp_msm_g1_mont_dev over the resident powers_of_g1;
  * aggregate_proofs: zkp_fr_asvc_subset_weights_dev, then one variable-base MSM;
  * all_proofs_key / prove_all: all n single-position proofs from three zkp_g1_ntt_dev transforms (one of them once per key), one
    zkp_g1_scale_vec_dev and two zkp_ntt_dev transforms (Tomescu et al. §3.4, after Feist-Khovratovich); lagrange_from_powers:
    l_of_g1 from the powers of tau with one inverse zkp_g1_ntt_dev, without the trapdoor;
  * the updates: their few scalars are host integers, the point work one variable-base MSM; the *_many forms prepare their m scalars
    on the device (powers of w gathered at the changed positions, element-wise products, one batch inversion) and run one
    zkp_msm_g1_var_batch_dev call.

Points are (xy, inf): affine Montgomery words and the identity flag; scalars are Python integers.  There is no CPU fallback.
The verifiers do not run here; tests/asvc_ref.py has them in Python integers."""
from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np

from .api import NTT_FFT, NTT_IFFT, VEC_ADDC, VEC_MUL, VEC_SCALE
from .codec import fr_mont, fr_to_mont
from .params import get_curve

ASVC_MAX_POSITIONS = 1024      # ZKP_ASVC_MAX_POSITIONS
ASVC_THREADS = 256             # csrc/asvc.hpp: workgroup of every kernel
ASVC_GROUP = 4                 # positions that share one coefficient load in the segment-head pass
ASVC_SPAN = 8                  # consecutive quotient coefficients per thread of the output pass
ASVC_CHUNK = 32                # segment heads per thread of the scan
ASVC_TILE = ASVC_CHUNK * ASVC_THREADS
ASVC_MAX_LOG = 30
MSM_SMALL_MAX_G1 = 1 << 16     # ZKP_MSM_SMALL_MAX_G1: the *_many forms run one batched small MSM
G1_NTT_MAX_LOG = 24            # ZKP_G1_NTT_MAX_LOG
G1_NTT_LANES = 64              # csrc/g1_ntt.hpp: one wave per workgroup


def segment_length(k: int) -> int:
    """the L of zkp_fr_asvc_quotient_dev: 2^floor(log2 k)"""
    return 1 << (k.bit_length() - 1)


def domain_root(curve, n: int) -> int:
    """the w of zkp_ntt_dev's domain of size n (a power of two): ark's group_gen"""
    c = get_curve(curve)
    log_n = n.bit_length() - 1
    if n != 1 << log_n or log_n > c.two_adicity:
        raise ValueError("the domain is a power of two up to 2^two_adicity")
    return pow(pow(c.fr_generator, (c.r - 1) >> c.two_adicity, c.r), 1 << (c.two_adicity - log_n), c.r)


@dataclass
class UpdateKey:
    ai: np.ndarray
    ui: np.ndarray


@dataclass
class ProvingKey:
    """powers_of_g1: (n + 1, w); l_of_g1, a_i, u_i: (n, w) affine Montgomery (update_keys[i] = (a_i[i], u_i[i])); none is the identity"""
    curve: object
    n: int
    powers_of_g1: np.ndarray
    l_of_g1: np.ndarray
    a_i: np.ndarray
    u_i: np.ndarray
    l_bases: object = None
    p_bases: object = None
    ctx: object = None

    def update_key(self, i: int) -> UpdateKey:
        return UpdateKey(self.a_i[i], self.u_i[i])

    def upload(self, ctx) -> "ProvingKey":
        """l_of_g1 and powers_of_g1 become resident bases of `ctx`"""
        self.free()
        self.ctx = ctx
        self.l_bases = ctx.upload_bases(self.curve, 1, self.l_of_g1)
        self.p_bases = ctx.upload_bases(self.curve, 1, self.powers_of_g1)
        return self

    def free(self):
        for b in (self.l_bases, self.p_bases):
            if b is not None:
                b.free()
        self.l_bases = self.p_bases = None


@dataclass
class VerificationKey:
    powers_of_g1: np.ndarray
    powers_of_g2: np.ndarray
    a: np.ndarray


@dataclass
class Parameters:
    proving_key: ProvingKey
    verification_key: VerificationKey


def key_gen(ctx, curve, n: int, tau: int, g1, g2) -> Parameters:
    """n is rounded up to a power of two (at least 2); g1: (w,), g2: (2 w,) affine Montgomery generators.  tau in the domain
    (tau^n == 1) raises ValueError: a denominator tau - w^i would be zero."""
    c = get_curve(curve)
    r = c.r
    size = max(2, 1 << (int(n) - 1).bit_length())
    w = domain_root(c, size)
    tau %= r
    a_tau = (pow(tau, size, r) - 1) % r
    if a_tau == 0:
        raise ValueError("tau lies in the evaluation domain")
    one = fr_mont(1, c)
    raw_one = np.array([1, 0, 0, 0], dtype=np.uint64)               # SCALE by it: Montgomery -> canonical words
    bufs = [ctx.dev_alloc(32 * (size + 1)) for _ in range(6)]
    d_w, d_d, d_a, d_l, d_u, d_p = bufs
    try:
        ctx.fr_powers_dev(c, one, fr_mont(w, c), d_w, size)                       # w^i
        ctx.fr_vec_op(c, VEC_SCALE, d_w, None, d_d, size, fr_mont(r - 1, c))      # -w^i
        ctx.fr_vec_op(c, VEC_ADDC, d_d, None, d_d, size, fr_mont(tau, c))         # tau - w^i
        ctx.fr_batch_inverse(c, d_d, size)                                        # d_i
        ctx.fr_vec_op(c, VEC_SCALE, d_d, None, d_a, size, fr_mont(a_tau, c))      # a_i
        ctx.fr_vec_op(c, VEC_MUL, d_a, d_w, d_l, size)
        ctx.fr_vec_op(c, VEC_SCALE, d_l, None, d_l, size, fr_mont(pow(size, -1, r), c))   # l_i
        ctx.fr_vec_op(c, VEC_ADDC, d_l, None, d_u, size, fr_mont(r - 1, c))
        ctx.fr_vec_op(c, VEC_MUL, d_u, d_d, d_u, size)                            # u_i
        ctx.fr_powers_dev(c, one, fr_mont(tau, c), d_p, size + 1)                 # tau^j
        canon = {}
        for name, ptr, count in (("a", d_a, size), ("l", d_l, size), ("u", d_u, size), ("p", d_p, size + 1)):
            ctx.fr_vec_op(c, VEC_SCALE, ptr, None, ptr, count, raw_one)
            canon[name] = np.zeros((count, 4), dtype=np.uint64)
            ctx.d2h(canon[name], ptr)
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
    g1, g2 = np.ascontiguousarray(g1, dtype=np.uint64), np.ascontiguousarray(g2, dtype=np.uint64)
    p1, _ = ctx.fixed_base_mul(c, 1, g1, canon["p"])
    p2, _ = ctx.fixed_base_mul(c, 2, g2, canon["p"])
    a_pts, _ = ctx.fixed_base_mul(c, 1, g1, canon["a"])
    l_pts, _ = ctx.fixed_base_mul(c, 1, g1, canon["l"])
    u_pts, _ = ctx.fixed_base_mul(c, 1, g1, canon["u"])
    a_pt, _ = ctx.fixed_base_mul(c, 1, g1, np.array([[(a_tau >> (64 * j)) & (2 ** 64 - 1) for j in range(4)]], dtype=np.uint64))
    return Parameters(ProvingKey(c, size, p1, l_pts, a_pts, u_pts), VerificationKey(p1, p2, a_pt[0]))


def commit(pk: ProvingKey, values):
    """the commitment to `values` (1 <= len <= n): one MSM over the resident l_of_g1"""
    if not 1 <= len(values) <= pk.n:
        raise ValueError("between 1 and n values")
    ctx, c = pk.ctx, pk.curve
    d = ctx.to_device(fr_to_mont(values, c))
    try:
        return ctx.into_affine(c, 1, pk.l_bases.msm_mont_dev(d, len(values)))
    finally:
        ctx.dev_free(d)


def check_points(points, n: int):
    pts = [int(p) for p in points]
    if not 1 <= len(pts) <= min(n, ASVC_MAX_POSITIONS):
        raise ValueError(f"between 1 and min(n, {ASVC_MAX_POSITIONS}) positions")
    if len(set(pts)) != len(pts):
        raise ValueError("a position is repeated")
    if min(pts) < 0 or max(pts) >= n:
        raise ValueError("a position lies outside the domain")
    return pts


def prove_pos(pk: ProvingKey, values, points, stats: dict | None = None):
    """the proof for the subvector at `points`: inverse transform, quotient by A_I, MSM over the powers of tau.  All n positions give
    the identity.  stats (a dict) receives the host's wall seconds per stage."""
    ctx, c, n = pk.ctx, pk.curve, pk.n
    pts = check_points(points, n)
    if len(values) > n:
        raise ValueError("more values than the domain holds")
    k = len(pts)
    if k == n:
        return np.zeros(2 * c.fq_limbs, dtype=np.uint64), True
    log_n = n.bit_length() - 1
    clock = [time.perf_counter()]

    def lap(key):
        ctx.sync()
        now = time.perf_counter()
        if stats is not None:
            stats[key] = stats.get(key, 0.0) + now - clock[0]
        clock[0] = now

    padded = np.zeros((n, 4), dtype=np.uint64)
    padded[:len(values)] = fr_to_mont(values, c)
    d_phi, d_q = ctx.to_device(padded), ctx.dev_alloc(32 * (n - k))
    try:
        lap("upload")
        ctx.ntt_dev(c, d_phi, log_n, NTT_IFFT)
        lap("ifft")
        ctx.fr_asvc_quotient_dev(c, d_phi, log_n, pts, d_q)
        lap("quotient")
        jac = pk.p_bases.msm_mont_dev(d_q, n - k)
        lap("msm")
        out = ctx.into_affine(c, 1, jac)
        lap("affine")
        return out
    finally:
        ctx.sync()
        ctx.dev_free(d_phi)
        ctx.dev_free(d_q)


@dataclass
class AllProofsKey:
    """the resident table A of prove_all: the size-2n transform of (tau^(n-2), ..., tau, 1, 0, ..., 0) g1 as device points"""
    curve: object
    n: int
    ctx: object
    a_xy: int = 0
    a_inf: int = 0

    def free(self):
        for p in (self.a_xy, self.a_inf):
            if p:
                self.ctx.dev_free(p)
        self.a_xy = self.a_inf = 0


def _g1_log(c, size: int) -> int:
    log = size.bit_length() - 1
    if size != 1 << log or log < 1 or log > min(G1_NTT_MAX_LOG, c.two_adicity):
        raise ValueError(f"a G1 transform takes 2^1 .. 2^{min(G1_NTT_MAX_LOG, c.two_adicity)} points")
    return log


def all_proofs_key(ctx, pk: ProvingKey) -> AllProofsKey:
    """the key of prove_all: a_k = powers_of_g1[n-2-k] for k <= n-2 and the identity up to 2n, transformed once (size 2n)"""
    c, n = pk.curve, pk.n
    log2n = _g1_log(c, 2 * n)
    a = np.zeros((2 * n, 2 * c.fq_limbs), dtype=np.uint64)
    a[:n - 1] = np.asarray(pk.powers_of_g1, dtype=np.uint64)[n - 2::-1]
    flags = np.ones(2 * n, dtype=np.uint8)
    flags[:n - 1] = 0
    apk = AllProofsKey(c, n, ctx)
    try:
        apk.a_xy, apk.a_inf = ctx.to_device(a), ctx.to_device(flags)
        ctx.g1_ntt_dev(c, apk.a_xy, apk.a_inf, log2n, NTT_FFT)
        ctx.sync()
    except Exception:
        apk.free()
        raise
    return apk


def prove_all(pk: ProvingKey, apk: AllProofsKey, values, stats: dict | None = None):
    """every single-position proof at once: ((n, w) affine Montgomery, (n,) identity flags), proof i equal to
    prove_pos(pk, values, [i]) bit for bit.  With c the coefficients of the values' polynomial,
    q_i(tau) = sum_m w^(i m) h_m(tau) and h_m = sum_{j <= n-2-m} c_{m+1+j} tau^j = (a * b)_{n-1+m} for a = (tau^(n-2), ..., 1) and
    b = c, a linear convolution that the cyclic one of size 2n holds (degree <= 2n - 3): B = FFT_2n(c, 0 x n), conv =
    IFFT_2n(A_i B_i), proofs = FFT_n(conv[n-1 .. 2n-2]) (conv[2n-2] is the identity h_{n-1}).  stats (a dict) receives the host's
    wall seconds per stage."""
    ctx, c, n = apk.ctx, pk.curve, pk.n
    if apk.n != n or get_curve(apk.curve) is not get_curve(c) or not apk.a_xy:
        raise ValueError("the all-proofs key belongs to another proving key")
    if not 1 <= len(values) <= n:
        raise ValueError("between 1 and n values")
    log_n, log2n = n.bit_length() - 1, _g1_log(c, 2 * n)
    pb = 16 * c.fq_limbs                                                # bytes of one affine point
    clock = [time.perf_counter()]

    def lap(key):
        ctx.sync()
        now = time.perf_counter()
        if stats is not None:
            stats[key] = stats.get(key, 0.0) + now - clock[0]
        clock[0] = now

    padded = np.zeros((2 * n, 4), dtype=np.uint64)
    padded[:len(values)] = fr_to_mont(values, c)
    bufs = []
    try:
        bufs.append(ctx.to_device(padded))
        bufs.append(ctx.dev_alloc(2 * n * pb))
        bufs.append(ctx.dev_alloc(2 * n))
        d_b, d_xy, d_inf = bufs
        lap("upload")
        ctx.ntt_dev(c, d_b, log_n, NTT_IFFT)                            # c_0 .. c_{n-1}; the upper half stays zero
        lap("ifft")
        ctx.ntt_dev(c, d_b, log2n, NTT_FFT)                             # B
        lap("fft")
        ctx.g1_scale_vec_dev(c, apk.a_xy, apk.a_inf, d_b, 2 * n, d_xy, d_inf)
        lap("scale")
        ctx.g1_ntt_dev(c, d_xy, d_inf, log2n, NTT_IFFT)                 # conv
        lap("g1_ifft")
        ctx.g1_ntt_dev(c, d_xy + (n - 1) * pb, d_inf + n - 1, log_n, NTT_FFT)   # H -> the proofs, in place
        lap("g1_fft")
        out, inf = np.zeros((n, 2 * c.fq_limbs), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        ctx.d2h(out, d_xy + (n - 1) * pb)
        ctx.d2h(inf, d_inf + n - 1)
        lap("download")
        return out, inf
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)


def lagrange_from_powers(ctx, curve, powers_xy, n: int):
    """l_of_g1 from powers_of_g1[:n] without the trapdoor: L_i(tau) = (1/n) sum_j w^(-i j) tau^j is one inverse transform over G1.
    Returns ((n, w) affine Montgomery, (n,) identity flags)."""
    c = get_curve(curve)
    _g1_log(c, n)
    xy = np.ascontiguousarray(powers_xy, dtype=np.uint64)
    if xy.ndim != 2 or xy.shape[0] < n:
        raise ValueError("n powers of tau are needed")
    return ctx.g1_ntt(c, xy[:n], None, NTT_IFFT)


def _msm_points(ctx, c, points, scalars):
    """sum_i scalars[i] points[i] for a few (xy, inf) points and integer scalars: one variable-base MSM"""
    xy = np.stack([np.asarray(p[0], dtype=np.uint64) for p in points])
    inf = np.array([1 if p[1] else 0 for p in points], dtype=np.uint8)
    return ctx.into_affine(c, 1, ctx.msm_var(c, 1, xy, inf, fr_to_mont(scalars, c), montgomery=True))


def aggregate_proofs(ctx, curve, n: int, points, proofs):
    """one proof for the union of single-position proofs: sum_i c_i proofs[i], c_i from zkp_fr_asvc_subset_weights_dev"""
    c = get_curve(curve)
    pts = check_points(points, n)
    if len(proofs) != len(pts):
        raise ValueError("one proof per position")
    weights = ctx.fr_asvc_subset_weights_dev(c, n.bit_length() - 1, pts)
    xy = np.stack([np.asarray(p[0], dtype=np.uint64) for p in proofs])
    inf = np.array([1 if p[1] else 0 for p in proofs], dtype=np.uint8)
    return ctx.into_affine(c, 1, ctx.msm_var(c, 1, xy, inf, weights, montgomery=True))


def update_commit(ctx, curve, commitment, delta: int, point: int, upk: UpdateKey, n: int):
    """the commitment after values[point] += delta: commitment + [delta w^point / n] a_point"""
    c = get_curve(curve)
    s = delta * pow(domain_root(c, n), point, c.r) % c.r * pow(n, -1, c.r) % c.r
    return _msm_points(ctx, c, [commitment, (upk.ai, False)], [1, s])


def update_proof(ctx, curve, proof, delta: int, point_i: int, point_j: int, upk_i: UpdateKey, upk_j: UpdateKey, n: int):
    """the single-position proof at point_i after values[point_j] += delta"""
    c = get_curve(curve)
    r = c.r
    if point_i == point_j:
        return _msm_points(ctx, c, [proof, (upk_i.ui, False)], [1, delta])
    w = domain_root(c, n)
    wi, wj = pow(w, point_i, r), pow(w, point_j, r)
    s = delta * wj % r * pow(n, -1, r) % r
    c1 = pow((wj - wi) % r, -1, r)
    return _msm_points(ctx, c, [proof, (upk_j.ai, False), (upk_i.ai, False)], [1, s * c1, -s * c1])


def _changed_scalars(ctx, c, n: int, changes, bufs):
    """device vectors for m changes (position, delta): (w^p_j, delta_j w^p_j / n), Montgomery"""
    m = len(changes)
    if not 1 <= m < MSM_SMALL_MAX_G1 // 2:
        raise ValueError("between 1 and 32767 changes")
    pos = np.array([int(p) for p, _ in changes], dtype=np.int32)
    if pos.min() < 0 or pos.max() >= n:
        raise ValueError("a position lies outside the domain")

    def keep(p):
        bufs.append(p)
        return p

    d_pow, d_idx = keep(ctx.dev_alloc(32 * n)), keep(ctx.to_device(pos))
    d_wp, d_s = keep(ctx.dev_alloc(32 * m)), keep(ctx.to_device(fr_to_mont([d for _, d in changes], c)))
    ctx.fr_powers_dev(c, fr_mont(1, c), fr_mont(domain_root(c, n), c), d_pow, n)
    ctx.fr_gather(d_pow, d_idx, m, d_wp)                                          # w^p_j
    ctx.fr_vec_op(c, VEC_MUL, d_s, d_wp, d_s, m)
    ctx.fr_vec_op(c, VEC_SCALE, d_s, None, d_s, m, fr_mont(pow(n, -1, c.r), c))   # delta_j w^p_j / n
    return d_wp, d_s


def _points_to_device(ctx, xy_rows, bufs):
    d = ctx.to_device(np.stack([np.asarray(p, dtype=np.uint64) for p in xy_rows]))
    bufs.append(d)
    return d


def update_commit_many(ctx, curve, commitment, changes, upks, n: int):
    """the commitment after values[p] += delta for every (p, delta) of `changes` (positions may repeat); upks[j]: the update key
    of changes[j]'s position.  One MSM; equals update_commit applied change by change."""
    c = get_curve(curve)
    if len(upks) != len(changes):
        raise ValueError("one update key per change")
    if commitment[1]:
        raise ValueError("the commitment is the identity")          # the batched MSM takes flags per vector, not per call
    m, bufs = len(changes), []
    try:
        _, d_s = _changed_scalars(ctx, c, n, changes, bufs)
        d_sc = ctx.dev_alloc(32 * (m + 1))
        bufs.append(d_sc)
        ctx.h2d(d_sc, fr_mont(1, c))
        ctx.d2d(d_sc + 32, d_s, 32 * m)
        d_xy = _points_to_device(ctx, [commitment[0]] + [u.ai for u in upks], bufs)
        jac = ctx.msm_var_batch_dev(c, 1, [d_xy], None, [d_sc], [m + 1], montgomery=True)
        return ctx.into_affine(c, 1, jac[0])
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)


def update_proof_many(ctx, curve, proof, i: int, upk_i: UpdateKey, changes, upks, n: int):
    """the single-position proof at i after every (p, delta) of `changes`:
    proof += sum_{p_j != i} delta_j (w^p_j / n) (a_{p_j} - a_i) / (w^p_j - w^i)  +  (sum_{p_j == i} delta_j) u_i.
    One MSM; equals update_proof applied change by change."""
    c = get_curve(curve)
    r = c.r
    if len(upks) != len(changes):
        raise ValueError("one update key per change")
    if proof[1]:
        raise ValueError("the proof is the identity")
    m, bufs = len(changes), []
    try:
        d_wp, d_s = _changed_scalars(ctx, c, n, changes, bufs)
        wi = pow(domain_root(c, n), i, r)
        ctx.fr_vec_op(c, VEC_ADDC, d_wp, None, d_wp, m, fr_mont(r - wi, c))       # w^p_j - w^i: zero where p_j == i ...
        ctx.fr_batch_inverse(c, d_wp, m)                                          # ... and a zero stays zero
        d_sc = ctx.dev_alloc(32 * (2 * m + 2))
        bufs.append(d_sc)
        own = sum(d for p, d in changes if int(p) == i) % r
        ctx.h2d(d_sc, fr_to_mont([1, own], c))
        ctx.fr_vec_op(c, VEC_MUL, d_s, d_wp, d_sc + 64, m)                        # t_j on a_{p_j}
        ctx.fr_vec_op(c, VEC_SCALE, d_sc + 64, None, d_sc + 64 + 32 * m, m, fr_mont(r - 1, c))   # -t_j on a_i
        d_xy = _points_to_device(ctx, [proof[0], upk_i.ui] + [u.ai for u in upks] + [upk_i.ai] * m, bufs)
        jac = ctx.msm_var_batch_dev(c, 1, [d_xy], None, [d_sc], [2 * m + 2], montgomery=True)
        return ctx.into_affine(c, 1, jac[0])
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
