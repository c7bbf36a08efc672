"""zkp_g1_ipa_fold_dev / zkp_fr_dot_batch_dev / ipa.inner_product_prove on the device, against known discrete logs (ctx.fixed_base_mul),
the oracle/pyref group law, oracle/cpu's fr_dot, and a pure-Python IPA prover that follows spartan/src/inner_product.rs:35-88."""
import ctypes
import hashlib

import numpy as np
import pytest

from ckb_zkp_amd import codec, ipa
from ckb_zkp_amd.params import get_curve
from oracle import cpu_oracle
from oracle.pyref.curves import Group
from tests import glv_ref
from tests.util import OC, random_points, to_abi_points

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xABABABABABABABAB


def _rand(rng, c, n):
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)      # < 2^(bits - 1) < r
    return codec.limbs_to_ints(k)


def _mont(c, x):
    return codec.fr_to_mont([x], c)[0]


def _gen(curve):
    return to_abi_points(curve, 1, [Group(OC[curve], 1).gen])[0]


def _mul(ctx, c, g_xy, es):
    """e_i G as ((n, w) words, (n,) flags), written by zkp_fixed_base_mul_g1"""
    return ctx.fixed_base_mul(c, 1, g_xy, codec.fr_canonical(es, c))


@pytest.mark.parametrize("curve,n", [(cv, n) for cv in CURVES for n in (1, 2, 63, 64, 65, 1000, 1 << 16)] + [("bn254", 1 << 20)])
def test_known_dlogs(ctx, curve, n):
    c = get_curve(curve)
    rng = np.random.default_rng(n + (curve == "bls12_381"))
    g = _gen(curve)
    lv, rv = _rand(rng, c, n), _rand(rng, c, n)
    for i in range(0, n, 7):
        lv[i] = 0                                                 # identity flags on L
    for i in range(3, n, 11):
        rv[i] = 0
    if n > 5:
        lv[5] = rv[5] = 0                                         # both identities: the output is the identity
    L, Li = _mul(ctx, c, g, lv)
    R, Ri = _mul(ctx, c, g, rv)
    a, b = _rand(rng, c, 2)
    xy, inf = ctx.ipa_fold(c, L, Li, R, Ri, _mont(c, a), _mont(c, b))
    exy, einf = _mul(ctx, c, g, [(a * x + b * y) % c.r for x, y in zip(lv, rv)])
    assert np.array_equal(inf, einf)
    assert np.array_equal(xy, exy)


@pytest.mark.parametrize("curve", CURVES)
def test_against_pyref(ctx, curve):
    c = get_curve(curve)
    G = Group(OC[curve], 1)
    r = c.r
    P = random_points(curve, 1, 12, seed=3)
    Q = random_points(curve, 1, 12, seed=4)
    Q[6] = P[6]                                                   # L = R
    Q[7] = G.neg(P[7])                                            # L = -R, a = b: the identity
    P[8] = None                                                   # flagged identity
    cases = [(0, 5), (7, 0), (1, r - 1), (12345, 12345), (r - 1, 1), (2, 3), (9, 9), (4, 4), (3, 5), (0, 0), (r - 2, r - 3), (1, 1)]
    # the scalars at the edges of the GLV split of a and b (tests/test_glv_split.py): lambda, lambda + 1, r - lambda and the picks
    # of the CPU run (largest parts, zero parts, each reachable sign pair); these are checked in every column
    gl = glv_ref.Glv(curve)
    edge = [gl.lam, gl.lam + 1, r - gl.lam] + [e for _, e in glv_ref.GLV_EDGE[curve]]
    cases += [(e, edge[(i + 1) % len(edge)]) for i, e in enumerate(edge)] + [(e, e) for e in edge[:3]] + [(1, gl.lam), (gl.lam, 1)]
    L, Li = to_abi_points(curve, 1, P)
    R, Ri = to_abi_points(curve, 1, Q)
    for k, (a, b) in enumerate(cases):
        xy, inf = ctx.ipa_fold(c, L, Li, R, Ri, _mont(c, a), _mont(c, b))
        got = codec.g1_from_mont(xy, inf, c)
        for j in ([k] if k < 12 else range(12)):
            exp = G.add(G.mul(P[j], a) if P[j] else None, G.mul(Q[j], b))
            assert got[j] == exp, (k, j, a, b)
    xy, inf = ctx.ipa_fold(c, L, Li, R, Ri, _mont(c, 4), _mont(c, 4))
    assert inf[7] == 1 and not xy[7].any()


def _dev_pair(ctx, c, n, seed):
    rng = np.random.default_rng(seed)
    g = _gen(c.name)
    lv, rv = _rand(rng, c, n), _rand(rng, c, n)
    lv[1] = 0
    L, Li = _mul(ctx, c, g, lv)
    R, Ri = _mul(ctx, c, g, rv)
    return L, Li, R, Ri


@pytest.mark.parametrize("curve", CURVES)
def test_in_place_and_repeat(ctx, curve):
    c = get_curve(curve)
    n = 777
    L, Li, R, Ri = _dev_pair(ctx, c, n, 11)
    a, b = _mont(c, 1234567), _mont(c, 7654321)
    ref_xy, ref_inf = ctx.ipa_fold(c, L, Li, R, Ri, a, b)
    again = ctx.ipa_fold(c, L, Li, R, Ri, a, b)
    assert np.array_equal(again[0], ref_xy) and np.array_equal(again[1], ref_inf)
    for over in ("l", "r"):
        ptrs = [ctx.to_device(x) for x in (L, Li, R, Ri)]
        try:
            dl, dli, dr, dri = ptrs
            out, oi = (dl, dli) if over == "l" else (dr, dri)
            ctx.ipa_fold_dev(c, dl, dli, dr, dri, n, a, b, out, oi)
            xy, inf = np.zeros_like(L), np.zeros(n, dtype=np.uint8)
            ctx.d2h(xy, out)
            ctx.d2h(inf, oi)
            assert np.array_equal(xy, ref_xy) and np.array_equal(inf, ref_inf), over
        finally:
            for p in ptrs:
                ctx.dev_free(p)


@pytest.mark.parametrize("curve", CURVES)
def test_errors_leave_output_untouched(ctx, curve):
    c = get_curve(curve)
    n = 64
    L, Li, R, Ri = _dev_pair(ctx, c, n, 12)
    w = L.shape[1]
    ptrs = [ctx.to_device(x) for x in (L, Li, R, Ri)]
    dout = ctx.to_device(np.full((n + 2, w), SENT, dtype=np.uint64))
    doi = ctx.to_device(np.full(n + 16, 0xAB, dtype=np.uint8))
    fn = ctx.lib.zkp_g1_ipa_fold_dev
    V = ctypes.c_void_p
    good = _mont(c, 5)
    big = np.frombuffer(c.r.to_bytes(32, "little"), dtype=np.uint64).copy()      # r: not reduced
    try:
        dl, dli, dr, dri = ptrs
        kp = lambda a: V(a.ctypes.data)                           # noqa: E731
        base = dict(cu=c.cid, l=dl, li=dli, r=dr, ri=dri, n=n, a=good, b=good, o=dout, oi=doi)

        def call(**kw):
            a = dict(base, **kw)
            return fn(ctx.h, a["cu"], V(a["l"]), V(a["li"]), V(a["r"]), V(a["ri"]), a["n"], kp(a["a"]) if a["a"] is not None else None,
                      kp(a["b"]) if a["b"] is not None else None, V(a["o"]), V(a["oi"]))
        bad = [dict(l=0), dict(r=0), dict(o=0), dict(oi=0), dict(a=None), dict(b=None),       # NULL arrays
               dict(l=dl + 8), dict(r=dr + 8), dict(o=dout + 8),                                # misaligned
               dict(a=big), dict(b=big),                                                        # a, b >= r
               dict(o=dl + 16 * w), dict(o=dr + 8 * w),                                           # partial overlap with L / R
               dict(oi=dli + 1), dict(oi=dri + 3), dict(oi=dl), dict(o=dout, oi=dout + 64)]      # flags overlapping
        for kw in bad:
            assert call(**kw) == -1, kw
        assert call(cu=7) == -2
        assert call(n=0, l=0, r=0, a=None, b=None, o=0, oi=0) == 0
        chk = np.zeros((n + 2, w), dtype=np.uint64)
        ctx.d2h(chk, dout)
        chi = np.zeros(n + 16, dtype=np.uint8)
        ctx.d2h(chi, doi)
        assert (chk == SENT).all() and (chi == 0xAB).all()
        assert call() == 0
    finally:
        for p in ptrs + [dout, doi]:
            ctx.dev_free(p)


@pytest.mark.parametrize("curve", CURVES)
def test_fr_dot_batch(ctx, curve):
    c = get_curve(curve)
    rng = np.random.default_rng(21)
    ns = [0, 1, 5, 2047, 2048, 2049, 10000, 0, 300]
    N = 1 << 20 if curve == "bn254" else 20000
    A = codec.fr_to_mont(_rand(rng, c, N), c)
    B = codec.fr_to_mont(_rand(rng, c, N), c)
    da, db = ctx.to_device(A), ctx.to_device(B)
    try:
        offs = [(7 * k * k) % 5000 for k in range(len(ns))]
        ap = [da + 32 * o for o in offs] + [da, da, da + 32]                                  # the last three: aliased entries
        bp = [db + 32 * o for o in offs] + [db, da, da + 32]
        nn = ns + [N, 4096, 4096]
        out = ctx.fr_dot_batch_dev(c, ap, bp, nn)
        for k, n in enumerate(nn):
            a = A[offs[k]:offs[k] + n] if k < len(ns) else (A if k == len(ns) else A[k - len(ns) - 1:][:n])
            b = B[offs[k]:offs[k] + n] if k < len(ns) else (B if k == len(ns) else A[k - len(ns) - 1:][:n])
            exp = cpu_oracle.fr_dot(c, a, b) if n else 0
            assert codec.fr_from_mont(out[k], c)[0] == exp, k
        assert ctx.fr_dot_batch_dev(c, [], [], []).shape == (0, 4)
    finally:
        ctx.dev_free(da)
        ctx.dev_free(db)


# ------------------------------------------------------------------------------------------- whole IPA
def _challenge(c):
    def ch(l_xy, l_inf, r_xy, r_inf):
        h = hashlib.sha256(np.ascontiguousarray(l_xy).tobytes() + bytes([int(l_inf)]) + np.ascontiguousarray(r_xy).tobytes()
                           + bytes([int(r_inf)])).digest()
        return int.from_bytes(h, "little") % c.r or 1
    return ch


def _py_prove(c, G, g_pts, q, h, a, b, gamma, blinds, ch):
    """bullet_inner_product_proof (spartan/src/inner_product.rs:35-88) on oracle/pyref points and Python integers"""
    r = c.r
    words = lambda p: to_abi_points(c.name, 1, [p])                # noqa: E731
    a, b, g = list(a), list(b), list(g_pts)
    blind_fin = gamma
    l_vec, r_vec = [], []
    n = len(a)
    for bl_, br_ in blinds:
        if n == 1:
            break
        n //= 2
        al, ar, bl, br, gl, gr = a[:n], a[n:], b[:n], b[n:], g[:n], g[n:]
        cl = sum(x * y for x, y in zip(al, br)) % r
        cr = sum(x * y for x, y in zip(ar, bl)) % r
        L = G.msm_naive(gr + [q, h], al + [cl, bl_])
        R = G.msm_naive(gl + [q, h], ar + [cr, br_])
        l_vec.append(L)
        r_vec.append(R)
        lw, li = words(L)
        rw, ri = words(R)
        x = ch(lw[0], li[0], rw[0], ri[0])
        xi = pow(x, -1, r)
        g = [G.add(G.mul(gl[i], xi) if gl[i] else None, G.mul(gr[i], x) if gr[i] else None) for i in range(n)]
        a = [(al[i] * x + ar[i] * xi) % r for i in range(n)]
        b = [(bl[i] * xi + br[i] * x) % r for i in range(n)]
        blind_fin = (blind_fin + x * x * bl_ + xi * xi * br_) % r
    return l_vec, r_vec, a[0], b[0], g[0], blind_fin


@pytest.mark.parametrize("curve", CURVES)
def test_prove_small_matches_python(ctx, curve):
    c = get_curve(curve)
    G = Group(OC[curve], 1)
    n = 32
    rng = np.random.default_rng(31)
    g_pts = random_points(curve, 1, n, seed=40)
    g_pts[3] = None
    q, h = random_points(curve, 1, 2, seed=41)
    a, b = _rand(rng, c, n), _rand(rng, c, n)
    gamma = _rand(rng, c, 1)[0]
    blinds = [tuple(_rand(rng, c, 2)) for _ in range(5)]
    ch = _challenge(c)
    g_xy, g_inf = to_abi_points(curve, 1, g_pts)
    m = lambda xs: codec.fr_to_mont(xs, c)                         # noqa: E731
    lv, rv, af, bf, (gxy, ginf), bfin = ipa.inner_product_prove(
        ctx, c, g_xy, g_inf, to_abi_points(curve, 1, [q])[0][0], to_abi_points(curve, 1, [h])[0][0], m(a), m(b), m([gamma])[0],
        [(m([x])[0], m([y])[0]) for x, y in blinds], ch)
    el, er, ea, eb, eg, ebf = _py_prove(c, G, g_pts, q, h, a, b, gamma, blinds, ch)
    assert [codec.g1_from_mont(x, [i], c)[0] for x, i in lv] == el
    assert [codec.g1_from_mont(x, [i], c)[0] for x, i in rv] == er
    fr = lambda v: codec.fr_from_mont(v, c)[0]                     # noqa: E731
    assert (fr(af), fr(bf), fr(bfin)) == (ea, eb, ebf)
    assert codec.g1_from_mont(gxy, [ginf], c)[0] == eg


def test_prove_large_known_dlogs(ctx):
    curve = "bn254"
    c = get_curve(curve)
    r = c.r
    n = 1 << 16
    rng = np.random.default_rng(51)
    g = _gen(curve)
    d = _rand(rng, c, n)
    d[9] = 0
    dq, dh = _rand(rng, c, 2)
    g_xy, g_inf = _mul(ctx, c, g, d)
    qh, _ = _mul(ctx, c, g, [dq, dh])
    a, b = _rand(rng, c, n), _rand(rng, c, n)
    gamma = 17
    blinds = [tuple(_rand(rng, c, 2)) for _ in range(16)]
    ch = _challenge(c)
    m = lambda xs: codec.fr_to_mont(xs, c)                         # noqa: E731
    lv, rv, af, bf, (gxy, ginf), bfin = ipa.inner_product_prove(
        ctx, c, g_xy, g_inf, qh[0], qh[1], m(a), m(b), m([gamma])[0], [(m([x])[0], m([y])[0]) for x, y in blinds], ch)
    el, er = [], []
    k = n
    for j, (bl_, br_) in enumerate(blinds):
        k //= 2
        al, ar, bl, br, dl, dr = a[:k], a[k:], b[:k], b[k:], d[:k], d[k:]
        cl = sum(x * y for x, y in zip(al, br)) % r
        cr = sum(x * y for x, y in zip(ar, bl)) % r
        el.append((sum(x * y for x, y in zip(al, dr)) + cl * dq + bl_ * dh) % r)
        er.append((sum(x * y for x, y in zip(ar, dl)) + cr * dq + br_ * dh) % r)
        x = ch(lv[j][0], lv[j][1], rv[j][0], rv[j][1])
        xi = pow(x, -1, r)
        d = [(dl[i] * xi + dr[i] * x) % r for i in range(k)]
        a = [(al[i] * x + ar[i] * xi) % r for i in range(k)]
        b = [(bl[i] * xi + br[i] * x) % r for i in range(k)]
    exy, einf = _mul(ctx, c, g, el + er + d)
    for j in range(16):
        assert np.array_equal(lv[j][0], exy[j]) and lv[j][1] == bool(einf[j]), j
        assert np.array_equal(rv[j][0], exy[16 + j]) and rv[j][1] == bool(einf[16 + j]), j
    assert np.array_equal(gxy, exy[32]) and ginf == bool(einf[32])
    assert codec.fr_from_mont(af, c)[0] == a[0] and codec.fr_from_mont(bf, c)[0] == b[0]
