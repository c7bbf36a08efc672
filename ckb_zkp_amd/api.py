"""Thin object layer over the C ABI (numpy in / numpy out).  One `Context` per GPU / process."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .params import CurveParams, get_curve

NTT_FFT, NTT_IFFT, NTT_COSET_FFT, NTT_COSET_IFFT = 0, 1, 2, 3
SC_EQ_AB_MINUS_C, SC_PROD2, SC_PROD3 = 0, 1, 2            # zkp_sumcheck_kind
SC_ARITY = {SC_EQ_AB_MINUS_C: 4, SC_PROD2: 2, SC_PROD3: 3}
SC_POINTS = {SC_EQ_AB_MINUS_C: 3, SC_PROD2: 2, SC_PROD3: 3}


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return C.c_void_p(a.ctypes.data)


def _c64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)


class Context:
    """zkp_ctx: device, stream, twiddle tables, scratch, resident bases."""

    def __init__(self, device: int = 0, config=None):
        """config: None (defaults = environment) or a dict / _lib.CtxConfig of zkp_ctx_config fields for THIS context
        (zkp_ctx_create_ex), e.g. Context(0, dict(lanes=2, h_evaluation_form=False))."""
        self.lib = _lib.load()
        h = C.c_void_p()
        cfg = _lib.make_config(config)
        if cfg is None:
            _lib.check(self.lib.zkp_ctx_create(C.byref(h), device), "zkp_ctx_create")
        else:
            _lib.check(self.lib.zkp_ctx_create_ex(C.byref(h), device, C.byref(cfg)), "zkp_ctx_create_ex")
        self.h = h
        self.device = device

    def config(self) -> dict:
        """the resolved zkp_ctx_config of this context (zkp_ctx_get_config)"""
        cfg = _lib.CtxConfig()
        _lib.check(self.lib.zkp_ctx_get_config(self.h, C.byref(cfg)), "zkp_ctx_get_config")
        return {f[0]: getattr(cfg, f[0]) for f in _lib.CtxConfig._fields_}

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.zkp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- plumbing
    def set_stream(self, hip_stream: int | None):
        _lib.check(self.lib.zkp_ctx_set_stream(self.h, C.c_void_p(hip_stream or 0)), "zkp_ctx_set_stream")

    def sync(self):
        _lib.check(self.lib.zkp_ctx_sync(self.h), "zkp_ctx_sync")

    def set_profiling(self, on: bool):
        _lib.check(self.lib.zkp_set_profiling(self.h, 1 if on else 0), "zkp_set_profiling")

    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _lib.check(self.lib.zkp_dev_alloc(self.h, nbytes, C.byref(p)), "zkp_dev_alloc")
        return p.value

    def dev_free(self, dptr: int):
        _lib.check(self.lib.zkp_dev_free(self.h, C.c_void_p(dptr)), "zkp_dev_free")

    def h2d(self, dptr: int, a: np.ndarray):
        a = np.ascontiguousarray(a)
        _lib.check(self.lib.zkp_h2d(self.h, C.c_void_p(dptr), _ptr(a), a.nbytes), "zkp_h2d")

    def d2h(self, a: np.ndarray, dptr: int):
        assert a.flags["C_CONTIGUOUS"]
        _lib.check(self.lib.zkp_d2h(self.h, _ptr(a), C.c_void_p(dptr), a.nbytes), "zkp_d2h")

    def to_device(self, a: np.ndarray) -> int:
        a = np.ascontiguousarray(a)
        d = self.dev_alloc(a.nbytes)
        self.h2d(d, a)
        return d

    def timer_start(self):
        _lib.check(self.lib.zkp_timer_start(self.h), "zkp_timer_start")

    def timer_stop_ms(self) -> float:
        ms = C.c_float()
        _lib.check(self.lib.zkp_timer_stop_ms(self.h, C.byref(ms)), "zkp_timer_stop_ms")
        return ms.value

    def bench_mulmod(self, curve, field: int, unsaturated: bool) -> float:
        """zkp_bench_mulmod: sustained 1e9 Montgomery products / s of the library's multiplier (field 0 = Fr, 1 = Fq)"""
        g = C.c_double()
        _lib.check(self.lib.zkp_bench_mulmod(self.h, get_curve(curve).cid, field, 1 if unsaturated else 0, C.byref(g)),
                   "zkp_bench_mulmod")
        return g.value

    def bench_hbm_copy(self, nbytes: int = 2 << 30) -> float:
        """zkp_bench_hbm_copy: GB/s (read + written) of a streaming copy kernel on this device"""
        g = C.c_double()
        _lib.check(self.lib.zkp_bench_hbm_copy(self.h, nbytes, C.byref(g)), "zkp_bench_hbm_copy")
        return g.value

    # ---- NTT (ark-poly EvaluationDomain ops)
    def ntt(self, curve, data: np.ndarray, op: int) -> np.ndarray:
        """data: (2^k, 4) uint64 Montgomery Fr; returns the transformed copy."""
        c = get_curve(curve)
        a = _c64(data).copy()
        n = a.shape[0]
        assert n & (n - 1) == 0 and a.shape[1] == 4
        _lib.check(self.lib.zkp_ntt(self.h, c.cid, _ptr(a), n.bit_length() - 1, op), "zkp_ntt")
        return a

    def ntt_dev(self, curve, dptr: int, log_n: int, op: int):
        _lib.check(self.lib.zkp_ntt_dev(self.h, get_curve(curve).cid, C.c_void_p(dptr), log_n, op), "zkp_ntt_dev")

    # ---- bases / MSM (ark-ec VariableBaseMSM)
    def upload_bases(self, curve, group: int, xy: np.ndarray, inf: np.ndarray | None = None) -> "Bases":
        c = get_curve(curve)
        xy = _c64(xy)
        n = xy.shape[0] if xy.ndim == 2 else 0
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
        hnd = C.c_uint64()
        fn = self.lib.zkp_bases_upload_g1 if group == 1 else self.lib.zkp_bases_upload_g2
        _lib.check(fn(self.h, c.cid, _ptr(xy), _ptr(inf), n, C.byref(hnd)), "zkp_bases_upload")
        return Bases(self, c, group, hnd.value, n)

    def msm_var(self, curve, group: int, xy: np.ndarray, inf, scalars: np.ndarray, montgomery: bool = False) -> np.ndarray:
        """zkp_msm_g*_var: true variable-base MSM (fresh host bases, nothing resident) -> Jacobian limbs."""
        c = get_curve(curve)
        xy, s = _c64(xy), _c64(scalars)
        n = min(xy.shape[0] if xy.ndim == 2 else 0, s.shape[0] if s.ndim == 2 else 0)
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
        out = np.zeros(3 * c.fq_limbs * (1 if group == 1 else 2), dtype=np.uint64)
        fn = self.lib.zkp_msm_g1_var if group == 1 else self.lib.zkp_msm_g2_var
        _lib.check(fn(self.h, c.cid, _ptr(xy), _ptr(inf), _ptr(s), n, 1 if montgomery else 0, _ptr(out)), "zkp_msm_var")
        return out

    def msm_var_batch_dev(self, curve, group: int, xy_ptrs, inf_ptrs, scalar_ptrs, ns, montgomery: bool = False) -> np.ndarray:
        """zkp_msm_g*_var_batch_dev: len(ns) independent small variable-base MSMs over DEVICE pointers (inf_ptrs None, or a list
        with None / 0 for entries without identity flags) -> (count, words) Jacobian limbs."""
        c = get_curve(curve)
        k = len(ns)
        words = 3 * c.fq_limbs * (1 if group == 1 else 2)
        out = np.zeros((k, words), dtype=np.uint64)
        xa = (C.c_void_p * max(k, 1))(*[p or None for p in xy_ptrs])
        sa = (C.c_void_p * max(k, 1))(*[p or None for p in scalar_ptrs])
        ia = None if inf_ptrs is None else (C.c_void_p * max(k, 1))(*[p or None for p in inf_ptrs])
        na = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        fn = self.lib.zkp_msm_g1_var_batch_dev if group == 1 else self.lib.zkp_msm_g2_var_batch_dev
        _lib.check(fn(self.h, c.cid, k, xa, ia, sa, na, 1 if montgomery else 0, _ptr(out)), "zkp_msm_var_batch_dev")
        return out

    def msm_var_batch(self, curve, group: int, xys, infs, scalars, montgomery: bool = False) -> np.ndarray:
        """Host convenience over msm_var_batch_dev: lists of numpy arrays (infs None, or a list with None entries) are uploaded,
        run as one batch and freed.  Entry k uses min(len(xys[k]), len(scalars[k])) terms, as msm_var does."""
        k = len(xys)
        assert len(scalars) == k and (infs is None or len(infs) == k)
        bufs, xp, ip, sp, ns = [], [], [], [], []
        try:
            for i in range(k):
                xy, s = _c64(xys[i]), _c64(scalars[i])
                n = min(xy.shape[0] if xy.ndim == 2 else 0, s.shape[0] if s.ndim == 2 else 0)
                ns.append(n)
                px = ps = pi = None
                if n:
                    px = self.to_device(xy[:n])
                    bufs.append(px)
                    ps = self.to_device(s[:n])
                    bufs.append(ps)
                    if infs is not None and infs[i] is not None:
                        pi = self.to_device(np.ascontiguousarray(infs[i], dtype=np.uint8)[:n])
                        bufs.append(pi)
                xp.append(px)
                sp.append(ps)
                ip.append(pi)
            return self.msm_var_batch_dev(curve, group, xp, None if infs is None else ip, sp, ns, montgomery)
        finally:
            for p in bufs:
                self.dev_free(p)

    def ipa_fold_dev(self, curve, l_xy_dev: int, l_inf_dev, r_xy_dev: int, r_inf_dev, n: int, a_mont, b_mont, out_xy_dev: int,
                     out_inf_dev: int):
        """zkp_g1_ipa_fold_dev: out[i] = (a L[i] + b R[i]).into_affine() over DEVICE pointers (G1; flags None / 0 = none; out may
        equal L or R); a_mont, b_mont: one Fr element each, Montgomery (4 x u64)."""
        a, b = _c64(a_mont), _c64(b_mont)
        _lib.check(self.lib.zkp_g1_ipa_fold_dev(self.h, get_curve(curve).cid, C.c_void_p(l_xy_dev or 0), C.c_void_p(l_inf_dev or 0),
                                                C.c_void_p(r_xy_dev or 0), C.c_void_p(r_inf_dev or 0), n, _ptr(a), _ptr(b),
                                                C.c_void_p(out_xy_dev or 0), C.c_void_p(out_inf_dev or 0)), "zkp_g1_ipa_fold_dev")

    def ipa_fold(self, curve, l_xy: np.ndarray, l_inf, r_xy: np.ndarray, r_inf, a_mont, b_mont):
        """Host convenience over ipa_fold_dev: ((n, w) affine Montgomery, (n,) identity flags) of a L[i] + b R[i]."""
        l_xy, r_xy = _c64(l_xy), _c64(r_xy)
        n = l_xy.shape[0]
        assert r_xy.shape == l_xy.shape
        out = np.zeros_like(l_xy)
        inf = np.zeros(n, dtype=np.uint8)
        if n == 0:
            return out, inf
        bufs = []
        try:
            def up(a):
                d = self.to_device(a)
                bufs.append(d)
                return d
            li = None if l_inf is None else up(np.ascontiguousarray(l_inf, dtype=np.uint8)[:n])
            ri = None if r_inf is None else up(np.ascontiguousarray(r_inf, dtype=np.uint8)[:n])
            dl, dr, do, di = up(l_xy), up(r_xy), up(out), up(inf)
            self.ipa_fold_dev(curve, dl, li, dr, ri, n, a_mont, b_mont, do, di)
            self.d2h(out, do)
            self.d2h(inf, di)
            return out, inf
        finally:
            for p in bufs:
                self.dev_free(p)

    def g1_scale_vec_dev(self, curve, xy_dev: int, inf_dev, scalars_dev: int, n: int, out_xy_dev: int, out_inf_dev: int):
        """zkp_g1_scale_vec_dev: out[i] = [s_i] P_i over DEVICE pointers (G1; flags None / 0 = none; scalars Montgomery Fr; out may
        equal the input).  Launches only."""
        _lib.check(self.lib.zkp_g1_scale_vec_dev(self.h, get_curve(curve).cid, C.c_void_p(xy_dev or 0), C.c_void_p(inf_dev or 0),
                                                 C.c_void_p(scalars_dev or 0), n, C.c_void_p(out_xy_dev or 0),
                                                 C.c_void_p(out_inf_dev or 0)), "zkp_g1_scale_vec_dev")

    def g1_ntt_dev(self, curve, xy_dev: int, inf_dev: int, log_n: int, op: int):
        """zkp_g1_ntt_dev: the transform over 2^log_n G1 points in place over DEVICE pointers (op NTT_FFT / NTT_IFFT, the root of
        ntt_dev; flags required).  Launches only."""
        _lib.check(self.lib.zkp_g1_ntt_dev(self.h, get_curve(curve).cid, C.c_void_p(xy_dev or 0), C.c_void_p(inf_dev or 0), log_n, op),
                   "zkp_g1_ntt_dev")

    def _g1_points_run(self, xy: np.ndarray, inf, extra, run):
        """upload (n, w) points, (n,) flags (None = none) and the arrays of `extra`, call run(d_xy, d_inf, *d_extra), download"""
        xy = _c64(xy)
        n = xy.shape[0]
        flags = np.zeros(n, dtype=np.uint8) if inf is None else np.ascontiguousarray(inf, dtype=np.uint8)[:n].copy()
        out = xy.copy()
        bufs = []
        try:
            for a in [out, flags] + [np.ascontiguousarray(e) for e in extra]:
                bufs.append(self.to_device(a))
            run(*bufs)
            self.d2h(out, bufs[0])
            self.d2h(flags, bufs[1])
            return out, flags
        finally:
            for p in bufs:
                self.dev_free(p)

    def g1_scale_vec(self, curve, xy: np.ndarray, inf, scalars_mont: np.ndarray):
        """Host convenience over g1_scale_vec_dev: ((n, w) affine Montgomery, (n,) identity flags) of [s_i] P_i."""
        s = _c64(scalars_mont)
        n = _c64(xy).shape[0]
        assert s.shape == (n, 4)
        if n == 0:
            return _c64(xy).copy(), np.zeros(0, dtype=np.uint8)
        return self._g1_points_run(xy, inf, [s], lambda d, di, ds: self.g1_scale_vec_dev(curve, d, di, ds, n, d, di))

    def g1_ntt(self, curve, xy: np.ndarray, inf, op: int):
        """Host convenience over g1_ntt_dev: the transformed copy of (2^k, w) points and their identity flags."""
        n = _c64(xy).shape[0]
        assert n >= 2 and n & (n - 1) == 0
        return self._g1_points_run(xy, inf, [], lambda d, di: self.g1_ntt_dev(curve, d, di, n.bit_length() - 1, op))

    # ---- optimal-ate pairings (ark-ec PairingEngine::{miller_loop, final_exponentiation, product_of_pairings})
    def pairing_info(self, curve) -> dict:
        """zkp_pairing_info: the power k of the final exponentiation's contract and the launch shape (no device work)."""
        info = (C.c_uint64 * 8)()
        _lib.check(self.lib.zkp_pairing_info(get_curve(curve).cid, info), "zkp_pairing_info")
        return dict(gt_power=info[0], fq12_words=info[1], pairs_per_workgroup=info[2], max_n=info[3], lds_bytes=info[4])

    def pairing_miller_dev(self, curve, g1_xy_dev: int, g1_inf_dev: int, g2_xy_dev: int, g2_inf_dev: int, n: int, group: int,
                           out_f12_dev: int):
        """zkp_pairing_miller_dev: out[j] = the product of the Miller functions of group j's pairs, over DEVICE pointers (affine
        Montgomery points + identity flags, both flag arrays required; n / group Fq12 out).  Launches only."""
        _lib.check(self.lib.zkp_pairing_miller_dev(self.h, get_curve(curve).cid, C.c_void_p(g1_xy_dev or 0), C.c_void_p(g1_inf_dev or 0),
                                                   C.c_void_p(g2_xy_dev or 0), C.c_void_p(g2_inf_dev or 0), n, group,
                                                   C.c_void_p(out_f12_dev or 0)), "zkp_pairing_miller_dev")

    def pairing_final_exp_dev(self, curve, f12_dev: int, m: int, out_gt_dev: int):
        """zkp_pairing_final_exp_dev: out[e] = f[e]^(k (q^12 - 1) / r) over m DEVICE Fq12 (out may be the input).  Launches only."""
        _lib.check(self.lib.zkp_pairing_final_exp_dev(self.h, get_curve(curve).cid, C.c_void_p(f12_dev or 0), m,
                                                      C.c_void_p(out_gt_dev or 0)), "zkp_pairing_final_exp_dev")

    def pairing_product_is_one_dev(self, curve, g1_xy_dev: int, g1_inf_dev: int, g2_xy_dev: int, g2_inf_dev: int, n: int, group: int,
                                   ok_dev: int):
        """zkp_pairing_product_is_one_dev: ok[j] = 1 iff the product of group j's pairings is one (n / group bytes).  Launches only."""
        _lib.check(self.lib.zkp_pairing_product_is_one_dev(self.h, get_curve(curve).cid, C.c_void_p(g1_xy_dev or 0),
                                                           C.c_void_p(g1_inf_dev or 0), C.c_void_p(g2_xy_dev or 0),
                                                           C.c_void_p(g2_inf_dev or 0), n, group, C.c_void_p(ok_dev or 0)),
                   "zkp_pairing_product_is_one_dev")

    def _pairing_args(self, c, g1_xy, g1_inf, g2_xy, g2_inf):
        g1, g2 = _c64(g1_xy).reshape(-1, 2 * c.fq_limbs), _c64(g2_xy).reshape(-1, 4 * c.fq_limbs)
        n = g1.shape[0]
        assert g2.shape[0] == n
        i1 = np.zeros(n, dtype=np.uint8) if g1_inf is None else np.ascontiguousarray(g1_inf, dtype=np.uint8)
        i2 = np.zeros(n, dtype=np.uint8) if g2_inf is None else np.ascontiguousarray(g2_inf, dtype=np.uint8)
        assert i1.shape == (n,) and i2.shape == (n,)
        return g1, i1, g2, i2, n

    def pairing(self, curve, g1_xy, g1_inf, g2_xy, g2_inf) -> np.ndarray:
        """zkp_pairing: (n, 12 * fq_limbs) uint64, row i = e(P_i, Q_i)^k as Montgomery words (flags None = no identities)."""
        c = get_curve(curve)
        g1, i1, g2, i2, n = self._pairing_args(c, g1_xy, g1_inf, g2_xy, g2_inf)
        out = np.zeros((n, 12 * c.fq_limbs), dtype=np.uint64)
        _lib.check(self.lib.zkp_pairing(self.h, c.cid, _ptr(g1), _ptr(i1), _ptr(g2), _ptr(i2), n, _ptr(out)), "zkp_pairing")
        return out

    def pairing_check(self, curve, g1_xy, g1_inf, g2_xy, g2_inf, group: int) -> np.ndarray:
        """zkp_pairing_check: (n / group,) uint8, entry j = 1 iff the product of group j's pairings is one."""
        c = get_curve(curve)
        g1, i1, g2, i2, n = self._pairing_args(c, g1_xy, g1_inf, g2_xy, g2_inf)
        ok = np.zeros(n // group if group and n % group == 0 else 1, dtype=np.uint8)
        _lib.check(self.lib.zkp_pairing_check(self.h, c.cid, _ptr(g1), _ptr(i1), _ptr(g2), _ptr(i2), n, group, _ptr(ok)),
                   "zkp_pairing_check")
        return ok

    def fr_dot_batch_dev(self, curve, a_ptrs, b_ptrs, ns) -> np.ndarray:
        """zkp_fr_dot_batch_dev: <a_k, b_k> over DEVICE Fr vectors (Montgomery) -> (count, 4) uint64 Montgomery."""
        k = len(ns)
        out = np.zeros((k, 4), dtype=np.uint64)
        aa = (C.c_void_p * max(k, 1))(*[p or None for p in a_ptrs])
        ba = (C.c_void_p * max(k, 1))(*[p or None for p in b_ptrs])
        na = (C.c_size_t * max(k, 1))(*[int(n) for n in ns])
        _lib.check(self.lib.zkp_fr_dot_batch_dev(self.h, get_curve(curve).cid, k, aa, ba, na, _ptr(out)), "zkp_fr_dot_batch_dev")
        return out

    def fr_sumcheck_round_dev(self, curve, kind: int, tables, length: int, bind=None, want_evals: bool = True):
        """zkp_fr_sumcheck_round_dev over DEVICE tables of `length` Fr each (Montgomery): `tables` is the flat list of
        count * arity(kind) pointers, term by term (SC_EQ_AB_MINUS_C: eq, a, b, c; SC_PROD2: a, b; SC_PROD3: a, b, c).
        bind: one Montgomery Fr (4 x u64) bound into every distinct table first (length halves), or None.
        Returns the (count, npoints) x 4 uint64 Montgomery evaluations g(0), g(2), (g(3)) per term, or None without want_evals."""
        ar, npts = SC_ARITY[kind], SC_POINTS[kind]
        assert len(tables) % ar == 0
        count = len(tables) // ar
        ta = (C.c_void_p * max(len(tables), 1))(*[p or None for p in tables])
        x = None if bind is None else _c64(bind)
        out = np.zeros((count, npts, 4), dtype=np.uint64) if want_evals else None
        _lib.check(self.lib.zkp_fr_sumcheck_round_dev(self.h, get_curve(curve).cid, kind, count, ta, length, _ptr(x), _ptr(out)),
                   "zkp_fr_sumcheck_round_dev")
        return out

    def fr_eq_evals_dev(self, curve, rs, out_ptr: int):
        """zkp_fr_eq_evals_dev: the 2^k table of eq(., rs) into DEVICE memory; rs: (k, 4) uint64 Montgomery, rs[0] the top index bit."""
        rs = _c64(rs).reshape(-1, 4)
        _lib.check(self.lib.zkp_fr_eq_evals_dev(self.h, get_curve(curve).cid, _ptr(rs) if rs.shape[0] else None, rs.shape[0],
                                                C.c_void_p(out_ptr or 0)), "zkp_fr_eq_evals_dev")

    def fr_eq_evals(self, curve, rs) -> np.ndarray:
        """Host convenience over fr_eq_evals_dev: (2^k, 4) uint64 Montgomery."""
        rs = _c64(rs).reshape(-1, 4)
        out = np.zeros((1 << rs.shape[0], 4), dtype=np.uint64)
        d = self.dev_alloc(out.nbytes)
        try:
            self.fr_eq_evals_dev(curve, rs, d)
            self.d2h(out, d)
            return out
        finally:
            self.dev_free(d)

    def fr_product_circuit_dev(self, curve, circuits, n: int) -> np.ndarray:
        """zkp_fr_product_circuit_dev: the layers above layer 0 of len(circuits) product circuits of n leaves each (DEVICE buffers
        of 2n - 2 Fr, layer l at element 2n - (2n >> l)) -> the (count, 4) uint64 Montgomery roots."""
        k = len(circuits)
        roots = np.zeros((k, 4), dtype=np.uint64)
        ca = (C.c_void_p * max(k, 1))(*[p or None for p in circuits])
        _lib.check(self.lib.zkp_fr_product_circuit_dev(self.h, get_curve(curve).cid, k, ca, n, _ptr(roots)), "zkp_fr_product_circuit_dev")
        return roots

    def fr_memcheck_circuits_dev(self, curve, addrs, vals, tss, ts_add, circuits, n: int, gamma1, gamma2) -> np.ndarray:
        """zkp_fr_memcheck_circuits_dev: leaf[i] = addr[i] gamma1^2 + val[i] gamma1 + ts[i] + ts_add - gamma2 as layer 0 of each
        circuit, then the circuits.  addrs / tss: DEVICE pointers to n uint32 or None (addr[i] = i / ts[i] = 0); vals: DEVICE
        pointers to n Montgomery Fr; ts_add: 0 or 1 per circuit; gamma1 / gamma2: one Montgomery Fr (4 x u64) each.
        Returns the (count, 4) uint64 Montgomery roots."""
        k = len(circuits)
        assert len(addrs) == len(vals) == len(tss) == len(ts_add) == k
        roots = np.zeros((k, 4), dtype=np.uint64)
        arr = lambda ps: (C.c_void_p * max(k, 1))(*[p or None for p in ps])    # noqa: E731
        ta = (C.c_uint32 * max(k, 1))(*[int(a) for a in ts_add])
        _lib.check(self.lib.zkp_fr_memcheck_circuits_dev(self.h, get_curve(curve).cid, k, arr(addrs), arr(vals), arr(tss), ta,
                                                         arr(circuits), n, _ptr(_c64(gamma1)), _ptr(_c64(gamma2)), _ptr(roots)),
                   "zkp_fr_memcheck_circuits_dev")
        return roots

    def gkr_layer_upload(self, op, left, right, log_in: int) -> int:
        """zkp_gkr_layer_upload: the wiring of one layer (op 0 = add / 1 = mul, left / right < 2^log_in) -> handle"""
        op = np.ascontiguousarray(op, dtype=np.uint8)
        left, right = np.ascontiguousarray(left, dtype=np.uint32), np.ascontiguousarray(right, dtype=np.uint32)
        assert len(op) == len(left) == len(right)
        h = C.c_void_p()
        _lib.check(self.lib.zkp_gkr_layer_upload(self.h, _ptr(op), _ptr(left), _ptr(right), len(op), log_in, C.byref(h)),
                   "zkp_gkr_layer_upload")
        return h.value

    def gkr_layer_free(self, layer: int):
        _lib.check(self.lib.zkp_gkr_layer_free(self.h, C.c_void_p(layer)), "zkp_gkr_layer_free")

    def gkr_layer_info(self, layer: int) -> dict:
        """zkp_gkr_layer_info: n_gates, log_out, log_in, n_mul, max_fan_left, max_fan_right, long_left, long_right"""
        info = (C.c_uint64 * 8)()
        _lib.check(self.lib.zkp_gkr_layer_info(C.c_void_p(layer), info), "zkp_gkr_layer_info")
        return dict(zip(("n_gates", "log_out", "log_in", "n_mul", "max_fan_left", "max_fan_right", "long_left", "long_right"),
                        (int(v) for v in info)))

    def fr_gkr_eval_layer_dev(self, curve, layer: int, in_ptr: int, out_ptr: int):
        """zkp_fr_gkr_eval_layer_dev: out[g] = in[left] (+ or *) in[right], zeros up to 2^log_out; DEVICE Montgomery Fr"""
        _lib.check(self.lib.zkp_fr_gkr_eval_layer_dev(self.h, get_curve(curve).cid, C.c_void_p(layer), C.c_void_p(in_ptr or 0),
                                                      C.c_void_p(out_ptr or 0)), "zkp_fr_gkr_eval_layer_dev")

    def fr_gkr_tables_dev(self, curve, layer: int, phase: int, g_ptr: int, w_ptr: int, outs):
        """zkp_fr_gkr_tables_dev: phase 1 (eval_hg): outs = mul, add1, add2 by left node, w = V; phase 2 (eval_fgu): outs = mul, add
        by right node, w = eq(ru).  Everything DEVICE Montgomery Fr: g 2^log_out, w and each output 2^log_in."""
        outs = list(outs) + [None] * (3 - len(outs))
        oa = (C.c_void_p * 3)(*[p or None for p in outs])
        _lib.check(self.lib.zkp_fr_gkr_tables_dev(self.h, get_curve(curve).cid, C.c_void_p(layer), phase, C.c_void_p(g_ptr or 0),
                                                  C.c_void_p(w_ptr or 0), oa), "zkp_fr_gkr_tables_dev")

    def fr_gkr_round_dev(self, curve, phase: int, tables, length: int, fu=None, bind=None, want_evals: bool = True):
        """zkp_fr_gkr_round_dev over DEVICE tables of `length` Fr (phase 1: f, mul, add1, add2; phase 2: f, mul, add and the
        Montgomery constant fu).  bind: one Montgomery Fr bound into every table first (length halves), or None.
        Returns the (2, 4) uint64 Montgomery g(0), g(2), or None without want_evals."""
        assert len(tables) == (4 if phase == 1 else 3)
        ta = (C.c_void_p * len(tables))(*[p or None for p in tables])
        x = None if bind is None else _c64(bind)
        f = None if fu is None else _c64(fu)
        out = np.zeros((2, 4), dtype=np.uint64) if want_evals else None
        _lib.check(self.lib.zkp_fr_gkr_round_dev(self.h, get_curve(curve).cid, phase, ta, length, _ptr(f), _ptr(x), _ptr(out)),
                   "zkp_fr_gkr_round_dev")
        return out

    def fr_gkr_eval_layer_batch_dev(self, curve, layer: int, in_ptr: int, out_ptr: int, n: int):
        """zkp_fr_gkr_eval_layer_batch_dev: one layer over n copies, node-major DEVICE Montgomery Fr: out[g n + t] =
        in[left n + t] (+ or *) in[right n + t], zero rows up to 2^log_out"""
        _lib.check(self.lib.zkp_fr_gkr_eval_layer_batch_dev(self.h, get_curve(curve).cid, C.c_void_p(layer), C.c_void_p(in_ptr or 0),
                                                            C.c_void_p(out_ptr or 0), n), "zkp_fr_gkr_eval_layer_batch_dev")

    def fr_gkr_dp_round_dev(self, curve, layer: int, v_ptr: int, eq_ptr: int, w_ptr: int, n: int, length: int, bind=None,
                            want_evals: bool = True, finals_ptr: int = 0):
        """zkp_fr_gkr_dp_round_dev: one round of Hyrax's sum-check over the copies.  v: 2^log_in rows of stride n, eq: n, w: 2^log_out
        DEVICE Montgomery Fr; `length` live.  bind: one Montgomery Fr bound into every row and eq first (length halves), or None.
        finals_ptr: 2^log_in Fr that receive element 0 of every row (only when the bound length is 1).
        Returns the (3, 4) uint64 Montgomery g(0), g(2), g(3), or None without want_evals."""
        x = None if bind is None else _c64(bind)
        out = np.zeros((3, 4), dtype=np.uint64) if want_evals else None
        _lib.check(self.lib.zkp_fr_gkr_dp_round_dev(self.h, get_curve(curve).cid, C.c_void_p(layer), C.c_void_p(v_ptr or 0),
                                                    C.c_void_p(eq_ptr or 0), C.c_void_p(w_ptr or 0), n, length, _ptr(x), _ptr(out),
                                                    C.c_void_p(finals_ptr or 0)), "zkp_fr_gkr_dp_round_dev")
        return out

    def fr_powers_dev(self, curve, first, ratio, out_ptr: int, n: int):
        """zkp_fr_powers_dev: out[i] = first ratio^i for i < n into DEVICE memory; first, ratio: one Montgomery Fr (4 x u64) each."""
        _lib.check(self.lib.zkp_fr_powers_dev(self.h, get_curve(curve).cid, _ptr(_c64(first)), _ptr(_c64(ratio)), C.c_void_p(out_ptr or 0), n),
                   "zkp_fr_powers_dev")

    @staticmethod
    def bp_vectors(aL: int, aR: int, aO: int, w: int, v: int, sL: int, sR: int, n: int, n_w: int, n_s: int, N: int) -> "_lib.BpVectors":
        """zkp_bp_vectors from DEVICE pointers (None / 0 where the length is 0) and lengths"""
        return _lib.BpVectors(aL or None, aR or None, aO or None, w or None, v or None, sL or None, sR or None, n, n_w, n_s, N)

    def fr_bp_t_coeffs_dev(self, curve, vecs, y, z) -> np.ndarray:
        """zkp_fr_bp_t_coeffs_dev: t2 .. t10 of <l(X), r(X)> as (9, 4) uint64 Montgomery; vecs: bp_vectors(...); y, z: Montgomery Fr."""
        out = np.zeros((9, 4), dtype=np.uint64)
        _lib.check(self.lib.zkp_fr_bp_t_coeffs_dev(self.h, get_curve(curve).cid, C.byref(vecs), _ptr(_c64(y)), _ptr(_c64(z)), _ptr(out)),
                   "zkp_fr_bp_t_coeffs_dev")
        return out

    def fr_bp_lr_eval_dev(self, curve, vecs, y, z, x, l_x_ptr: int, r_x_ptr: int) -> np.ndarray:
        """zkp_fr_bp_lr_eval_dev: l(x) and r(x) into the DEVICE buffers of N Fr each; returns t_x = <l(x), r(x)> ((4,) Montgomery)."""
        out = np.zeros(4, dtype=np.uint64)
        _lib.check(self.lib.zkp_fr_bp_lr_eval_dev(self.h, get_curve(curve).cid, C.byref(vecs), _ptr(_c64(y)), _ptr(_c64(z)), _ptr(_c64(x)),
                                                  C.c_void_p(l_x_ptr or 0), C.c_void_p(r_x_ptr or 0), _ptr(out)), "zkp_fr_bp_lr_eval_dev")
        return out

    def fr_ipa_fold_ab_dev(self, curve, a_ptr: int, b_ptr: int, n: int, x, want_c: bool = True):
        """zkp_fr_ipa_fold_ab_dev: a[j] = x a[j] + x^-1 a[j + n/2], b[j] = x^-1 b[j] + x b[j + n/2] in place over DEVICE Montgomery Fr.
        Returns the next round's (cL, cR) as (2, 4) uint64 Montgomery, or None without want_c or when n == 2."""
        out = np.zeros((2, 4), dtype=np.uint64) if want_c and n > 2 else None
        _lib.check(self.lib.zkp_fr_ipa_fold_ab_dev(self.h, get_curve(curve).cid, C.c_void_p(a_ptr or 0), C.c_void_p(b_ptr or 0), n,
                                                   _ptr(_c64(x)), _ptr(out)), "zkp_fr_ipa_fold_ab_dev")
        return out

    def fr_asvc_subset_weights_dev(self, curve, log_n: int, positions, out_ptr: int = 0, want_host: bool = True):
        """zkp_fr_asvc_subset_weights_dev: c_i = 1 / prod_{j != i} (w^p_i - w^p_j) for the distinct positions p_i < 2^log_n, into the
        DEVICE buffer out_ptr (k Fr, 0: none) and / or returned as (k, 4) uint64 Montgomery (None without want_host)."""
        pos = np.ascontiguousarray(positions, dtype=np.uint32)
        out = np.zeros((len(pos), 4), dtype=np.uint64) if want_host else None
        _lib.check(self.lib.zkp_fr_asvc_subset_weights_dev(self.h, get_curve(curve).cid, log_n, _ptr(pos), len(pos),
                                                           C.c_void_p(out_ptr or 0), _ptr(out)), "zkp_fr_asvc_subset_weights_dev")
        return out

    def fr_asvc_quotient_dev(self, curve, phi_ptr: int, log_n: int, positions, q_ptr: int):
        """zkp_fr_asvc_quotient_dev: q = floor(Phi / prod_i (X - w^p_i)) over DEVICE Montgomery Fr: 2^log_n coefficients in,
        2^log_n - k out.  Launches only."""
        pos = np.ascontiguousarray(positions, dtype=np.uint32)
        _lib.check(self.lib.zkp_fr_asvc_quotient_dev(self.h, get_curve(curve).cid, C.c_void_p(phi_ptr or 0), log_n, _ptr(pos), len(pos),
                                                     C.c_void_p(q_ptr or 0)), "zkp_fr_asvc_quotient_dev")
        self.sync()                                               # `pos` is host memory of this call

    def pedersen_key_create(self, curve, gens_xy, gens_inf, h_xy) -> int:
        """zkp_pedersen_key_create: the resident window tables of the (n, w) affine Montgomery generators (flags None = none) and
        the blinding generator h -> key handle (free it with pedersen_key_free)."""
        xy, h = _c64(gens_xy), _c64(h_xy)
        n = xy.shape[0] if xy.ndim == 2 else 0
        infa = None if gens_inf is None else np.ascontiguousarray(gens_inf, dtype=np.uint8)
        assert infa is None or infa.shape[0] >= n
        key = C.c_void_p()
        _lib.check(self.lib.zkp_pedersen_key_create(self.h, get_curve(curve).cid, _ptr(xy), _ptr(infa), n, _ptr(h), C.byref(key)),
                   "zkp_pedersen_key_create")
        return key.value

    def pedersen_key_free(self, key: int):
        _lib.check(self.lib.zkp_pedersen_key_free(self.h, C.c_void_p(key or 0)), "zkp_pedersen_key_free")

    def pedersen_key_info(self, key: int) -> dict:
        """zkp_pedersen_key_info -> n_gens, c, W, pairs_per_slice, gens_per_slice (G), table_bytes, lds_bytes, launches"""
        info = (C.c_uint64 * 8)()
        _lib.check(self.lib.zkp_pedersen_key_info(C.c_void_p(key or 0), info), "zkp_pedersen_key_info")
        return {"n_gens": info[0], "c": info[1], "W": info[2], "pairs_per_slice": info[3], "gens_per_slice": info[3] // info[2],
                "table_bytes": info[4], "lds_bytes": info[5], "launches": info[6]}

    def pedersen_commit_rows_dev(self, key: int, scalars_ptr: int, rows: int, cols: int, blinds_ptr, out_xy_ptr: int, out_inf_ptr: int):
        """zkp_pedersen_commit_rows_dev: out[i] = sum_j scalars[i cols + j] g_j + blinds[i] h over DEVICE Montgomery Fr (blinds None /
        0: no blind term) -> rows affine Montgomery points and flags in DEVICE memory.  Launches only."""
        _lib.check(self.lib.zkp_pedersen_commit_rows_dev(self.h, C.c_void_p(key or 0), C.c_void_p(scalars_ptr or 0), rows, cols,
                                                         C.c_void_p(blinds_ptr or 0), C.c_void_p(out_xy_ptr or 0),
                                                         C.c_void_p(out_inf_ptr or 0)), "zkp_pedersen_commit_rows_dev")

    def pedersen_commit_rows(self, curve, key: int, scalars_mont, blinds_mont=None):
        """Host convenience over pedersen_commit_rows_dev: (rows, cols, 4) Montgomery scalars and (rows, 4) blinds or None ->
        ((rows, w) affine Montgomery, (rows,) identity flags)."""
        s = _c64(scalars_mont)
        rows, cols = s.shape[0], s.shape[1]
        out = np.zeros((rows, 2 * get_curve(curve).fq_limbs), dtype=np.uint64)
        inf = np.zeros(rows, dtype=np.uint8)
        bufs = []
        try:
            def up(a):
                d = self.to_device(a)
                bufs.append(d)
                return d
            ds, do, di = up(s), up(out), up(inf)
            db = None if blinds_mont is None else up(_c64(blinds_mont))
            self.pedersen_commit_rows_dev(key, ds, rows, cols, db, do, di)
            self.d2h(out, do)
            self.d2h(inf, di)
            return out, inf
        finally:
            for p in bufs:
                self.dev_free(p)

    def fr_vecmat_dev(self, curve, l_ptr: int, m_ptr: int, rows: int, cols: int, out_ptr: int):
        """zkp_fr_vecmat_dev: out[j] = sum_i l[i] m[i cols + j] over DEVICE Montgomery Fr.  Launches only."""
        _lib.check(self.lib.zkp_fr_vecmat_dev(self.h, get_curve(curve).cid, C.c_void_p(l_ptr or 0), C.c_void_p(m_ptr or 0), rows, cols,
                                              C.c_void_p(out_ptr or 0)), "zkp_fr_vecmat_dev")

    def hash_params_create(self, curve, kind: int, rounds: int, constants, alpha: int = 0, mds=None, full_round=None,
                           inv_alpha: int = 0) -> int:
        """zkp_hash_params_create: constants / mds as Montgomery Fr words ((count, 4) uint64), full_round one byte per round,
        inv_alpha a plain integer -> params handle (free it with hash_params_free).  hashes.HashParams builds these from integers."""
        cs = _c64(constants)
        md = None if mds is None else _c64(mds)
        fl = None if full_round is None else np.ascontiguousarray(full_round, dtype=np.uint8)
        desc = _lib.HashDesc(C.sizeof(_lib.HashDesc), kind, rounds, alpha, _ptr(cs), _ptr(md), _ptr(fl),
                             (C.c_uint64 * 4)(*[(inv_alpha >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]))
        params = C.c_void_p()
        _lib.check(self.lib.zkp_hash_params_create(self.h, get_curve(curve).cid, C.byref(desc), C.byref(params)), "zkp_hash_params_create")
        return params.value

    def hash_params_free(self, params: int):
        _lib.check(self.lib.zkp_hash_params_free(self.h, C.c_void_p(params or 0)), "zkp_hash_params_free")

    def hash_params_info(self, params: int) -> dict:
        """zkp_hash_params_info -> kind, curve, rounds, device_bytes, alpha, products (Fr products of one block)"""
        info = (C.c_uint64 * 8)()
        _lib.check(self.lib.zkp_hash_params_info(C.c_void_p(params or 0), info), "zkp_hash_params_info")
        return {"kind": info[0], "curve": info[1], "rounds": info[2], "device_bytes": info[3], "alpha": info[4], "products": info[5]}

    def fr_hash_blocks_dev(self, params: int, xl_ptr: int, xr_ptr: int, n: int, out_ptr: int):
        """zkp_fr_hash_blocks_dev: out[k] = block(xl[k], xr[k]) over DEVICE Montgomery Fr; out may be xl or xr.  Launches only."""
        _lib.check(self.lib.zkp_fr_hash_blocks_dev(self.h, C.c_void_p(params or 0), C.c_void_p(xl_ptr or 0), C.c_void_p(xr_ptr or 0), n,
                                                   C.c_void_p(out_ptr or 0)), "zkp_fr_hash_blocks_dev")

    def fr_hash_chain_dev(self, params: int, msgs_ptr: int, n: int, length: int, out_ptr: int, xl_out_ptr: int = 0):
        """zkp_fr_hash_chain_dev: the reference's `*_hash` over n row-major messages of `length` elements; out[k] the image,
        xl_out[k] (0: not wanted) the state before the last block.  Launches only."""
        _lib.check(self.lib.zkp_fr_hash_chain_dev(self.h, C.c_void_p(params or 0), C.c_void_p(msgs_ptr or 0), n, length,
                                                  C.c_void_p(out_ptr or 0), C.c_void_p(xl_out_ptr or 0)), "zkp_fr_hash_chain_dev")

    def fr_mimc_trace_dev(self, params: int, xl_ptr: int, xr_ptr: int, n: int, out_ptr: int, stride: int):
        """zkp_fr_mimc_trace_dev: per block xl, xr, then (tmp, new_xl) per round at out + k * stride elements.  Launches only."""
        _lib.check(self.lib.zkp_fr_mimc_trace_dev(self.h, C.c_void_p(params or 0), C.c_void_p(xl_ptr or 0), C.c_void_p(xr_ptr or 0), n,
                                                  C.c_void_p(out_ptr or 0), stride), "zkp_fr_mimc_trace_dev")

    def fr_merkle_tree_dev(self, params: int, merge: int, nodes_ptr: int, n: int):
        """zkp_fr_merkle_tree_dev: fills the inner nodes [0, n - 1) of the 2 n - 1 nodes whose leaves sit at [n - 1, 2 n - 1)."""
        _lib.check(self.lib.zkp_fr_merkle_tree_dev(self.h, C.c_void_p(params or 0), merge, C.c_void_p(nodes_ptr or 0), n),
                   "zkp_fr_merkle_tree_dev")

    def fr_merkle_paths_dev(self, nodes_ptr: int, n: int, leaf_idx_ptr: int, q: int, out_ptr: int, stride: int, len_ptr: int):
        """zkp_fr_merkle_paths_dev: the siblings above q leaves (uint32 indices in DEVICE memory) into rows of `stride` elements and
        their counts (0xFFFFFFFF: the index is not a leaf).  One launch."""
        _lib.check(self.lib.zkp_fr_merkle_paths_dev(self.h, C.c_void_p(nodes_ptr or 0), n, C.c_void_p(leaf_idx_ptr or 0), q,
                                                    C.c_void_p(out_ptr or 0), stride, C.c_void_p(len_ptr or 0)), "zkp_fr_merkle_paths_dev")

    def sha256_dev(self, msgs_ptr: int, n: int, length: int, out_ptr: int):
        """zkp_sha256_dev: the digests of n row-major DEVICE messages of `length` bytes, 32 bytes each.  One launch."""
        _lib.check(self.lib.zkp_sha256_dev(self.h, C.c_void_p(msgs_ptr or 0), n, length, C.c_void_p(out_ptr or 0)), "zkp_sha256_dev")

    def sha256_trace_dev(self, msgs_ptr: int, n: int, length: int, trace_ptr: int):
        """zkp_sha256_trace_dev: the canonical trace of the same messages, sha256.trace_words(length) * n uint32.  One launch."""
        _lib.check(self.lib.zkp_sha256_trace_dev(self.h, C.c_void_p(msgs_ptr or 0), n, length, C.c_void_p(trace_ptr or 0)),
                   "zkp_sha256_trace_dev")

    def sha256_merkle_tree_dev(self, nodes_ptr: int, n: int):
        """zkp_sha256_merkle_tree_dev: fills the inner nodes [0, n - 1) of 2 n - 1 items of 32 bytes, the leaves at [n - 1, 2 n - 1)."""
        _lib.check(self.lib.zkp_sha256_merkle_tree_dev(self.h, C.c_void_p(nodes_ptr or 0), n), "zkp_sha256_merkle_tree_dev")

    def fr_bits_expand_dev(self, curve, trace_ptr: int, words_per_msg: int, msgs_per_instance: int, q: int, code_ptr: int, m: int,
                           max_v: int, z_ptr: int, z_stride: int):
        """zkp_fr_bits_expand_dev: z[b * z_stride + j] = the bit that code[j] selects from instance b's messages, as Montgomery 0 / 1."""
        _lib.check(self.lib.zkp_fr_bits_expand_dev(self.h, get_curve(curve).cid, C.c_void_p(trace_ptr or 0), words_per_msg,
                                                   msgs_per_instance, q, C.c_void_p(code_ptr or 0), m, max_v, C.c_void_p(z_ptr or 0),
                                                   z_stride), "zkp_fr_bits_expand_dev")

    def fr_prefix_product_dev(self, curve, in_ptr: int, out_ptr: int, n: int, want_total: bool = True):
        """zkp_fr_prefix_product_dev: out[0] = 1, out[i] = in[0] ... in[i-1] over n DEVICE Montgomery Fr (out may be in).
        Returns the (4,) uint64 Montgomery product of all n, or None without want_total."""
        total = np.zeros(4, dtype=np.uint64) if want_total else None
        _lib.check(self.lib.zkp_fr_prefix_product_dev(self.h, get_curve(curve).cid, C.c_void_p(in_ptr or 0), C.c_void_p(out_ptr or 0), n,
                                                      _ptr(total)), "zkp_fr_prefix_product_dev")
        return total

    def fr_plonk_perm_z_dev(self, curve, w_ptrs, sigma_ptrs, log_n: int, ks, beta, gamma, z_out_ptr: int) -> bool:
        """zkp_fr_plonk_perm_z_dev: the permutation accumulator z over 2^log_n rows into z_out.  w_ptrs / sigma_ptrs: 4 DEVICE
        tables each; ks (4, 4), beta, gamma (4,): uint64 Montgomery.  Returns `closes` (z[n-1] perm[n-1] == 1)."""
        assert len(w_ptrs) == 4 and len(sigma_ptrs) == 4
        wa = (C.c_void_p * 4)(*[p or None for p in w_ptrs])
        sa = (C.c_void_p * 4)(*[p or None for p in sigma_ptrs])
        closes = C.c_int32(-1)
        _lib.check(self.lib.zkp_fr_plonk_perm_z_dev(self.h, get_curve(curve).cid, wa, sa, log_n, _ptr(_c64(ks)), _ptr(_c64(beta)),
                                                    _ptr(_c64(gamma)), C.c_void_p(z_out_ptr or 0), C.byref(closes)),
                   "zkp_fr_plonk_perm_z_dev")
        return closes.value == 1

    def fr_plonk_quotient_dev(self, curve, w_ptrs, z_ptr: int, pi_ptr: int, q_ptrs, sigma_ptrs, l1_ptr: int, log_n: int, ks, beta,
                              gamma, alpha, t_out_ptr: int):
        """zkp_fr_plonk_quotient_dev: t = (t_arith + t_perm) v_4n_inversed over the 4 * 2^log_n coset points, one launch.
        q_ptrs: q_0, q_1, q_2, q_3, q_m, q_c, q_arith.  Every table DEVICE Montgomery Fr; t_out overlaps no input."""
        assert len(w_ptrs) == 4 and len(sigma_ptrs) == 4 and len(q_ptrs) == 7
        wa = (C.c_void_p * 4)(*[p or None for p in w_ptrs])
        sa = (C.c_void_p * 4)(*[p or None for p in sigma_ptrs])
        qa = (C.c_void_p * 7)(*[p or None for p in q_ptrs])
        _lib.check(self.lib.zkp_fr_plonk_quotient_dev(self.h, get_curve(curve).cid, wa, C.c_void_p(z_ptr or 0), C.c_void_p(pi_ptr or 0),
                                                      qa, sa, C.c_void_p(l1_ptr or 0), log_n, _ptr(_c64(ks)), _ptr(_c64(beta)),
                                                      _ptr(_c64(gamma)), _ptr(_c64(alpha)), C.c_void_p(t_out_ptr or 0)),
                   "zkp_fr_plonk_quotient_dev")

    def fr_poly_eval_many_dev(self, curve, p_ptrs, ns, z) -> np.ndarray:
        """zkp_fr_poly_eval_many_dev: the polynomials p_ptrs[k] (DEVICE Montgomery Fr, ns[k] coefficients; 0: the zero polynomial)
        at ONE point z ((4,) uint64 Montgomery).  Returns the (count, 4) uint64 Montgomery evaluations."""
        assert len(p_ptrs) == len(ns)
        count = len(ns)
        pa = (C.c_void_p * max(count, 1))(*[p or None for p in p_ptrs])
        na = (C.c_size_t * max(count, 1))(*ns)
        out = np.zeros((max(count, 1), 4), dtype=np.uint64)
        _lib.check(self.lib.zkp_fr_poly_eval_many_dev(self.h, get_curve(curve).cid, count, pa, na, _ptr(_c64(z)), _ptr(out)),
                   "zkp_fr_poly_eval_many_dev")
        return out[:count]

    def fr_lincomb_dev(self, curve, p_ptrs, ns, coeffs, out_ptr: int, n_out: int):
        """zkp_fr_lincomb_dev: out[i] = sum_{k : i < ns[k]} coeffs[k] p_k[i] for i < n_out, one launch.  p_ptrs / out: DEVICE
        Montgomery Fr; coeffs: (count, 4) uint64 Montgomery.  out may be one of the inputs itself."""
        assert len(p_ptrs) == len(ns)
        count = len(ns)
        pa = (C.c_void_p * max(count, 1))(*[p or None for p in p_ptrs])
        na = (C.c_size_t * max(count, 1))(*ns)
        ca = _c64(coeffs) if count else np.zeros((1, 4), dtype=np.uint64)
        assert ca.size == 4 * max(count, 1)
        _lib.check(self.lib.zkp_fr_lincomb_dev(self.h, get_curve(curve).cid, count, pa, na, _ptr(ca), C.c_void_p(out_ptr or 0), n_out),
                   "zkp_fr_lincomb_dev")

    def fold(self, curve, group: int, xyz: np.ndarray) -> np.ndarray:
        c = get_curve(curve)
        xyz = _c64(xyz)
        w = 3 * c.fq_limbs * (1 if group == 1 else 2)
        out = np.zeros(w, dtype=np.uint64)
        fn = self.lib.zkp_g1_fold if group == 1 else self.lib.zkp_g2_fold
        _lib.check(fn(self.h, c.cid, _ptr(xyz), xyz.size // w, _ptr(out)), "zkp_fold")
        return out

    def into_affine(self, curve, group: int, xyz: np.ndarray):
        c = get_curve(curve)
        w = 2 * c.fq_limbs * (1 if group == 1 else 2)
        xy = np.zeros(w, dtype=np.uint64)
        inf = np.zeros(1, dtype=np.uint8)
        fn = self.lib.zkp_g1_into_affine if group == 1 else self.lib.zkp_g2_into_affine
        _lib.check(fn(self.h, c.cid, _ptr(_c64(xyz)), _ptr(xy), _ptr(inf)), "zkp_into_affine")
        return xy, bool(inf[0])

    def decompress_points(self, curve, group: int, data: bytes):
        """zkp_g1/g2_decompress: ark-serialize compressed points -> ((n, w) affine Montgomery, (n,) identity flags).  Raises
        ValueError(index) on a malformed point."""
        c = get_curve(curve)
        pb = 8 * c.fq_limbs * (1 if group == 1 else 2)
        assert len(data) % pb == 0
        n = len(data) // pb
        w = 2 * c.fq_limbs * (1 if group == 1 else 2)
        xy = np.zeros((n, w), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        buf = np.frombuffer(data, dtype=np.uint8)
        bad = C.c_size_t(0)
        fn = self.lib.zkp_g1_decompress if group == 1 else self.lib.zkp_g2_decompress
        rc = fn(self.h, c.cid, _ptr(buf) if n else None, n, _ptr(xy), _ptr(inf), C.byref(bad))
        if rc == _lib.ZKP_ERR_INVALID_POINT:
            raise ValueError(f"malformed compressed point at index {bad.value}")
        _lib.check(rc, "zkp_decompress")
        return xy, inf

    def compress_points(self, curve, group: int, xy: np.ndarray, inf=None) -> bytes:
        """zkp_g1/g2_compress: affine Montgomery points -> ark-serialize compressed bytes"""
        c = get_curve(curve)
        xy = _c64(xy)
        n = xy.shape[0]
        pb = 8 * c.fq_limbs * (1 if group == 1 else 2)
        out = np.zeros(n * pb, dtype=np.uint8)
        infa = None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8)
        fn = self.lib.zkp_g1_compress if group == 1 else self.lib.zkp_g2_compress
        _lib.check(fn(self.h, c.cid, _ptr(xy), None if infa is None else _ptr(infa), n, _ptr(out)), "zkp_compress")
        return out.tobytes()

    def subgroup_check(self, curve, group: int, xy: np.ndarray, inf=None) -> None:
        """zkp_g1/g2_subgroup_check: every point on the curve and in the prime-order subgroup ([r]P = O), else ValueError(index) —
        the checked half of ark's `deserialize`."""
        c = get_curve(curve)
        xy = _c64(xy)
        n = xy.shape[0]
        infa = None if inf is None else np.ascontiguousarray(inf, dtype=np.uint8)
        bad = C.c_size_t(0)
        fn = self.lib.zkp_g1_subgroup_check if group == 1 else self.lib.zkp_g2_subgroup_check
        rc = fn(self.h, c.cid, _ptr(xy) if n else None, None if infa is None else _ptr(infa), n, C.byref(bad))
        if rc == _lib.ZKP_ERR_INVALID_POINT:
            raise ValueError(f"point {bad.value} is not in the prime-order subgroup (or not on the curve)")
        _lib.check(rc, "zkp_subgroup_check")

    def fixed_base_mul(self, curve, group: int, base_xy: np.ndarray, scalars: np.ndarray):
        """k_i * P for canonical scalars (n,4) -> ((n, w) uint64 affine Montgomery, (n,) uint8 identity flags)."""
        c = get_curve(curve)
        scalars = _c64(scalars)
        n = scalars.shape[0]
        w = 2 * c.fq_limbs * (1 if group == 1 else 2)
        out = np.zeros((n, w), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        fn = self.lib.zkp_fixed_base_mul_g1 if group == 1 else self.lib.zkp_fixed_base_mul_g2
        _lib.check(fn(self.h, c.cid, _ptr(_c64(base_xy)), _ptr(scalars), n, _ptr(out), _ptr(inf)), "zkp_fixed_base_mul")
        return out, inf


class Bases:
    """Device-resident query / SRS (zkp_bases_upload_*)."""

    def __init__(self, ctx: Context, curve: CurveParams, group: int, handle: int, n: int):
        self.ctx, self.curve, self.group, self.handle, self.n = ctx, curve, group, handle, n

    def free(self):
        if self.handle:
            _lib.check(self.ctx.lib.zkp_bases_free(self.ctx.h, self.handle), "zkp_bases_free")
            self.handle = 0

    def share_with(self, other_ctx: "Context") -> "Bases":
        """the same resident tables, addressable through another context (one context per prover thread)"""
        h = C.c_uint64(0)
        _lib.check(self.ctx.lib.zkp_bases_share(other_ctx.h, self.ctx.h, self.handle, C.byref(h)), "zkp_bases_share")
        return Bases(other_ctx, self.curve, self.group, h.value, self.n)

    def _out(self):
        return np.zeros(3 * self.curve.fq_limbs * (1 if self.group == 1 else 2), dtype=np.uint64)

    def msm(self, scalars: np.ndarray, offset: int = 0) -> np.ndarray:
        """VariableBaseMSM::multi_scalar_mul(bases[offset..], scalars) -> Jacobian (X,Y,Z) Montgomery limbs."""
        s = _c64(scalars)
        n = s.shape[0] if s.ndim == 2 else 0
        out = self._out()
        fn = self.ctx.lib.zkp_msm_g1 if self.group == 1 else self.ctx.lib.zkp_msm_g2
        _lib.check(fn(self.ctx.h, self.handle, offset, _ptr(s), n, _ptr(out)), "zkp_msm")
        return out

    def msm_dev(self, scalars_dev: int, n: int, offset: int = 0) -> np.ndarray:
        out = self._out()
        fn = self.ctx.lib.zkp_msm_g1_dev if self.group == 1 else self.ctx.lib.zkp_msm_g2_dev
        _lib.check(fn(self.ctx.h, self.handle, offset, C.c_void_p(scalars_dev), n, _ptr(out)), "zkp_msm_dev")
        return out

    def vartime_multiscalar_mul(self, fr_scalars_mont: np.ndarray) -> np.ndarray:
        """zkp_curve::Curve::vartime_multiscalar_mul (curve/src/lib.rs:38-45): Montgomery Fr scalars."""
        s = _c64(fr_scalars_mont)
        out = self._out()
        fn = self.ctx.lib.zkp_vartime_multiscalar_mul_g1 if self.group == 1 else \
            self.ctx.lib.zkp_vartime_multiscalar_mul_g2
        _lib.check(fn(self.ctx.h, self.handle, _ptr(s), s.shape[0] if s.ndim == 2 else 0, _ptr(out)),
                   "zkp_vartime_multiscalar_mul")
        return out

    def msm_affine(self, scalars: np.ndarray, offset: int = 0):
        return self.ctx.into_affine(self.curve, self.group, self.msm(scalars, offset))


# ---- Fr vector / polynomial primitives (device pointers), see include/zkp_accel.h
VEC_MUL, VEC_ADD, VEC_SUB, VEC_SCALE, VEC_AXPY, VEC_ADDC = 0, 1, 2, 3, 4, 5     # the `op` of fr_vec_op


def _ctx_method(fn):
    setattr(Context, fn.__name__, fn)
    return fn


@_ctx_method
def fr_vec_op(self, curve, op: int, a_dev: int, b_dev: int | None, out_dev: int, n: int, k_mont: np.ndarray | None = None):
    k = None if k_mont is None else _c64(k_mont)
    _lib.check(self.lib.zkp_fr_vec_op_dev(self.h, get_curve(curve).cid, op, C.c_void_p(a_dev),
                                          C.c_void_p(b_dev or 0), _ptr(k), C.c_void_p(out_dev), n), "zkp_fr_vec_op_dev")


@_ctx_method
def fr_batch_inverse(self, curve, v_dev: int, n: int):
    _lib.check(self.lib.zkp_fr_batch_inverse_dev(self.h, get_curve(curve).cid, C.c_void_p(v_dev), n),
               "zkp_fr_batch_inverse_dev")


@_ctx_method
def poly_evaluate(self, curve, p_dev: int, n: int, z_mont: np.ndarray) -> np.ndarray:
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(self.lib.zkp_poly_evaluate_dev(self.h, get_curve(curve).cid, C.c_void_p(p_dev), n, _ptr(_c64(z_mont)),
                                              _ptr(out)), "zkp_poly_evaluate_dev")
    return out


@_ctx_method
def poly_div_linear(self, curve, p_dev: int, n: int, z_mont: np.ndarray, q_dev: int) -> np.ndarray:
    out = np.zeros(4, dtype=np.uint64)
    _lib.check(self.lib.zkp_poly_div_linear_dev(self.h, get_curve(curve).cid, C.c_void_p(p_dev), n, _ptr(_c64(z_mont)),
                                                C.c_void_p(q_dev), _ptr(out)), "zkp_poly_div_linear_dev")
    return out


def _bases_msm_mont_dev(self, scalars_dev: int, n: int, offset: int = 0) -> np.ndarray:
    """MSM of device-resident Montgomery Fr scalars against bases[offset..] (KZG10 commit/open; sharded queries)."""
    out = self._out()
    fn = self.ctx.lib.zkp_msm_g1_mont_dev if self.group == 1 else self.ctx.lib.zkp_msm_g2_mont_dev
    _lib.check(fn(self.ctx.h, self.handle, offset, C.c_void_p(scalars_dev), n, _ptr(out)), "zkp_msm_mont_dev")
    return out


Bases.msm_mont_dev = _bases_msm_mont_dev


def _bases_msm_mont_batch_dev(self, jobs) -> np.ndarray:
    """PC::commit over a list: jobs = [(scalars_dev, n, offset)] -> (len(jobs), 3 * fq_limbs) Jacobian results; the MSMs
    run three at a time on the context's MSM streams."""
    assert self.group == 1
    k = len(jobs)
    out = np.zeros((k, 3 * self.curve.fq_limbs), dtype=np.uint64)
    if k == 0:
        return out
    ptrs = (C.c_void_p * k)(*[j[0] for j in jobs])
    ns = (C.c_size_t * k)(*[j[1] for j in jobs])
    offs = (C.c_size_t * k)(*[j[2] for j in jobs])
    _lib.check(self.ctx.lib.zkp_msm_g1_mont_batch_dev(self.ctx.h, self.handle, k, offs, ptrs, ns, _ptr(out)),
               "zkp_msm_g1_mont_batch_dev")
    return out


Bases.msm_mont_batch_dev = _bases_msm_mont_batch_dev


@_ctx_method
def fr_spmv(self, curve, row_ptr_dev: int, col_dev: int, coeff_dev: int, nrows: int, x_dev: int, out_dev: int):
    """out = M x for a CSR matrix resident in HBM (z_a = A z, and the transposed product behind Marlin's t)."""
    _lib.check(self.lib.zkp_fr_spmv_dev(self.h, get_curve(curve).cid, C.c_void_p(row_ptr_dev), C.c_void_p(col_dev),
                                        C.c_void_p(coeff_dev), nrows, C.c_void_p(x_dev), C.c_void_p(out_dev)),
               "zkp_fr_spmv_dev")


@_ctx_method
def fr_gather(self, in_dev: int, idx_dev: int, n: int, out_dev: int):
    _lib.check(self.lib.zkp_fr_gather_dev(self.h, C.c_void_p(in_dev), C.c_void_p(idx_dev), n, C.c_void_p(out_dev)),
               "zkp_fr_gather_dev")


@_ctx_method
def poly_divide_by_vanishing(self, curve, p_dev: int, length: int, n: int, q_dev: int | None, rem_dev: int | None):
    _lib.check(self.lib.zkp_poly_divide_by_vanishing_dev(self.h, get_curve(curve).cid, C.c_void_p(p_dev), length, n,
                                                         C.c_void_p(q_dev or 0), C.c_void_p(rem_dev or 0)),
               "zkp_poly_divide_by_vanishing_dev")


@_ctx_method
def d2d(self, dst_dev: int, src_dev: int, nbytes: int):
    _lib.check(self.lib.zkp_d2d(self.h, C.c_void_p(dst_dev), C.c_void_p(src_dev), nbytes), "zkp_d2d")


@_ctx_method
def dev_zero(self, dst_dev: int, nbytes: int):
    _lib.check(self.lib.zkp_dev_zero(self.h, C.c_void_p(dst_dev), nbytes), "zkp_dev_zero")


@_ctx_method
def msm_mont_multi_dev(self, jobs) -> list:
    """jobs = [(Bases, scalars_dev, n, offset)] with possibly different (G1 / G2) base vectors -> list of Jacobian limb
    arrays; the MSMs run four at a time on the context's MSM streams (zkp_msm_mont_multi_dev)."""
    k = len(jobs)
    if k == 0:
        return []
    slot = max(3 * b.curve.fq_limbs * (1 if b.group == 1 else 2) for b, *_ in jobs)
    out = np.zeros((k, slot), dtype=np.uint64)
    handles = (C.c_uint64 * k)(*[b.handle for b, *_ in jobs])
    ptrs = (C.c_void_p * k)(*[j[1] for j in jobs])
    ns = (C.c_size_t * k)(*[j[2] for j in jobs])
    offs = (C.c_size_t * k)(*[j[3] for j in jobs])
    _lib.check(self.lib.zkp_msm_mont_multi_dev(self.h, k, handles, offs, ptrs, ns, _ptr(out), slot), "zkp_msm_mont_multi_dev")
    return [out[i, :3 * b.curve.fq_limbs * (1 if b.group == 1 else 2)].copy() for i, (b, *_) in enumerate(jobs)]


class MultiContext(Context):
    """zkp_ctx_create_multi: ONE process, one context per listed device (ids may repeat on a one-GPU box), the exchange
    step of the base-sharded prover owned by the library.  The object itself is rank 0's context (usable like any
    Context); member(k) borrows rank k's."""

    def __init__(self, device_ids, config=None):
        self.lib = _lib.load()
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = C.c_void_p()
        cfg = _lib.make_config(config)
        _lib.check(self.lib.zkp_ctx_create_multi_ex(C.byref(h), ids, len(device_ids), C.byref(cfg) if cfg is not None else None),
                   "zkp_ctx_create_multi_ex")
        self.h = h
        self.device = device_ids[0]
        self.device_ids = list(device_ids)
        n = C.c_int32()
        _lib.check(self.lib.zkp_ctx_num_devices(self.h, C.byref(n)), "zkp_ctx_num_devices")
        assert n.value == len(device_ids)

    @property
    def num_devices(self) -> int:
        return len(self.device_ids)

    def member(self, rank: int) -> Context:
        m = C.c_void_p()
        _lib.check(self.lib.zkp_ctx_device(self.h, rank, C.byref(m)), "zkp_ctx_device")
        c = Context.__new__(Context)
        c.lib, c.h, c.device, c._borrowed = self.lib, m, self.device_ids[rank], True
        return c
