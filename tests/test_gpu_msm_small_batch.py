"""zkp_msm_g*_var_batch_dev: many independent small variable-base MSMs (fresh device bases) in one call, against the oracle
(oracle/pyref naive MSM, known discrete logs through oracle/cpu) and against the single-MSM variable-base path."""
import ctypes
import random
import threading
import time

import numpy as np
import pytest

from ckb_zkp_amd import codec
from ckb_zkp_amd.api import Context
from ckb_zkp_amd.params import get_curve
from oracle import cpu_oracle
from oracle.pyref.curves import Group
from tests.util import OC, jac_limbs_to_affine_oracle, random_points, to_abi_points

pytestmark = pytest.mark.gpu
CFG = [("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2)]
CAP = {1: 1 << 16, 2: 1 << 15}
R2 = 1 << 512


def _rand_fr(rng, c, n):
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)      # < 2^(bits - 1) < r
    return k


class Pool:
    """cap bases with known discrete logs (d = 0: the identity) and 2 cap scalars, on the host and on the device."""

    def __init__(self, ctx, curve, group, seed):
        self.c = c = get_curve(curve)
        self.curve, self.group = curve, group
        rng = np.random.default_rng(seed)
        n = CAP[group]
        self.d = _rand_fr(rng, c, n)
        self.d[5::997] = 0
        self.g_xy, _ = to_abi_points(curve, group, [Group(OC[curve], group).gen])
        self.xy, self.inf = ctx.fixed_base_mul(c, group, self.g_xy, self.d)
        assert self.inf[5] == 1
        self.k = _rand_fr(rng, c, 2 * n)
        self.ab = self.xy.shape[1] * 8
        self.ctx = ctx
        self.dxy, self.dinf, self.dk = ctx.to_device(self.xy), ctx.to_device(self.inf), ctx.to_device(self.k)

    def free(self):
        for p in (self.dxy, self.dinf, self.dk):
            self.ctx.dev_free(p)

    def entry(self, boff, soff, n):
        """device pointers of an entry: bases [boff, boff + n), scalars [soff, soff + n)"""
        return self.dxy + boff * self.ab, self.dinf + boff, self.dk + soff * 32, n

    def dlog(self, boff, soff, n, k=None):
        if n == 0:
            return 0
        ks = self.k[soff:soff + n] if k is None else k
        return cpu_oracle.fr_dot(self.c, self.d[boff:boff + n], ks) * R2 % self.c.r

    def expect(self, es):
        """e_k * G for every e_k, computed by the oracle (C++ fixed-base multiplication)"""
        xy, inf = cpu_oracle.fixed_base_mul(self.c.cid, self.group, self.g_xy, codec.fr_canonical(es, self.c))
        return (codec.g1_from_mont if self.group == 1 else codec.g2_from_mont)(xy, inf, self.c)

    def run(self, ctx, entries, inf=True, montgomery=False):
        return ctx.msm_var_batch_dev(self.c, self.group, [e[0] for e in entries], [e[1] for e in entries] if inf else None,
                                     [e[2] for e in entries], [e[3] for e in entries], montgomery)


_POOLS = {}


@pytest.fixture
def pool(ctx, curve, group):
    key = (curve, group)
    if key not in _POOLS:
        _POOLS[key] = Pool(ctx, curve, group, seed=91 + 2 * group + (curve == "bls12_381"))
    return _POOLS[key]


def _affine(curve, group, out):
    return [jac_limbs_to_affine_oracle(curve, group, row) for row in out]


@pytest.mark.parametrize("curve,group", CFG)
def test_edge_set_in_one_batch(ctx, curve, group):
    """The 24-point edge set of test_msm_var_true_variable_base_small (0, 1, r-1, 2, 2^253; an identity base; a duplicate base
    with an equal scalar; P and -P with equal scalars): entries of 24, 17, 1 and 0 points, one without identity flags, one with
    more scalars than points — one call, canonical and Montgomery scalars."""
    c = get_curve(curve)
    G = Group(OC[curve], group)
    rnd = random.Random(17)
    pts = random_points(curve, group, 24, seed=21 + group)
    pts[3] = None
    pts[5] = pts[4]
    pts[7] = G.neg(pts[6])
    ks = [rnd.randrange(c.r) for _ in range(24)]
    ks[0], ks[1], ks[2], ks[8], ks[9] = 0, 1, c.r - 1, 2, 1 << 253
    ks[5] = ks[4]
    ks[7] = ks[6]
    xy, inf = to_abi_points(curve, group, pts)
    sizes = (24, 17, 1, 0)
    exp = [G.msm_naive(pts[:n], ks[:n]) for n in sizes] + [G.msm_naive(pts[:3], ks[:3])]
    for mont in (False, True):
        enc = codec.fr_to_mont if mont else codec.fr_canonical
        xys = [xy[:n] for n in sizes] + [xy[:3]]
        infs = [inf[:n] for n in sizes] + [None]
        scs = [enc(ks[:n], c).reshape(-1, 4) for n in sizes] + [enc(ks[:9], c).reshape(-1, 4)]
        out = ctx.msm_var_batch(c, group, xys, infs, scs, montgomery=mont)
        assert out.shape == (5, 3 * c.fq_limbs * group)
        assert _affine(curve, group, out) == exp, mont
        # the C++ oracle agrees on the flagged entries
        for i, n in enumerate(sizes):
            ref = cpu_oracle.msm(c.cid, group, xy[:n], inf[:n], codec.fr_canonical(ks[:n], c).reshape(-1, 4))
            assert jac_limbs_to_affine_oracle(curve, group, ref) == exp[i]


@pytest.mark.parametrize("curve,group", CFG)
@pytest.mark.parametrize("count", [1, 7, 64, 300])
def test_random_batches_known_dlog(ctx, curve, group, count, pool):
    """Random ns[k] in [0, cap] over offsets into a pool of bases with known discrete logs (identity bases included); every
    result against e_k * G, a sample also against zkp_msm_g*_var on the same inputs."""
    cap = CAP[group]
    rnd = random.Random(count * 31 + group)
    entries, es = [], []
    for i in range(count):
        n = rnd.choice((0, 1, cap, rnd.randrange(cap + 1))) if i < 4 else rnd.randrange(cap + 1)
        boff, soff = rnd.randrange(cap - n + 1), rnd.randrange(cap + 1)
        entries.append(pool.entry(boff, soff, n) + (boff, soff))
        es.append(pool.dlog(boff, soff, n))
    mont = count == 7
    if mont:                                          # the same values in Montgomery form: a separate scalar array
        ints = codec.limbs_to_ints(pool.k)
        km = codec.fr_to_mont(ints, pool.c)
        dkm = ctx.to_device(km)
        entries = [(e[0], e[1], dkm + e[5] * 32, e[3], e[4], e[5]) for e in entries]
    try:
        out = pool.run(ctx, entries, montgomery=mont)
    finally:
        if mont:
            ctx.dev_free(dkm)
    assert _affine(curve, group, out) == pool.expect(es)
    for i in rnd.sample(range(count), min(count, 3)):
        _, _, _, n, boff, soff = entries[i]
        ref = ctx.msm_var(pool.c, group, pool.xy[boff:boff + n], pool.inf[boff:boff + n], pool.k[soff:soff + n])
        assert jac_limbs_to_affine_oracle(curve, group, ref) == jac_limbs_to_affine_oracle(curve, group, out[i])


@pytest.mark.parametrize("curve,group", CFG)
def test_skewed_scalars_at_cap(ctx, curve, group, pool):
    """n = cap with all scalars equal, all in {0, 1}, 300 equal among random ones, every 7th zero: right, and in the same
    order of time as random scalars of the same size (lanes split a long bucket; no lane walks it alone)."""
    n = CAP[group]
    rng = np.random.default_rng(5)
    base = pool.k[:n].copy()
    cases = {"random": base}
    eq = np.repeat(base[:1], n, axis=0)
    cases["equal"] = eq
    zo = np.zeros((n, 4), dtype=np.uint64)
    zo[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint64)
    cases["zero_one"] = zo
    k300 = base.copy()
    k300[100:400] = k300[99]
    cases["300_equal"] = k300
    k7 = base.copy()
    k7[::7] = 0
    cases["every_7th_zero"] = k7
    times = {}
    for name, k in cases.items():
        dk = ctx.to_device(k)
        try:
            ent = [(pool.dxy, pool.dinf, dk, n)]
            out = pool.run(ctx, ent)                  # warm-up and result
            t0 = time.perf_counter()
            for _ in range(3):
                pool.run(ctx, ent)
            times[name] = (time.perf_counter() - t0) / 3
        finally:
            ctx.dev_free(dk)
        assert _affine(curve, group, out) == pool.expect([pool.dlog(0, 0, n, k)]), name
    for name, t in times.items():
        assert t <= 10 * times["random"] + 0.02, (name, times)


@pytest.mark.parametrize("curve,group", CFG)
def test_aliasing(ctx, curve, group, pool):
    """One base vector shared by 32 entries with different scalars (hyrax L / R halves, commitment.rs:533-536), and one scalar
    vector shared by four base vectors."""
    n = 1000
    entries = [pool.entry(0, 37 * i, n) for i in range(32)]
    es = [pool.dlog(0, 37 * i, n) for i in range(32)]
    entries += [pool.entry(500 * i + 3, 11, n) for i in range(4)]
    es += [pool.dlog(500 * i + 3, 11, n) for i in range(4)]
    out = pool.run(ctx, entries)
    assert _affine(curve, group, out) == pool.expect(es)


@pytest.mark.parametrize("curve,group", CFG)
def test_caps_and_errors(ctx, curve, group, pool):
    """ns[k] = cap + 1 -> ZKP_ERR_BAD_ARG with the output untouched; count = 0 -> ZKP_OK; an entry at the cap works."""
    c = pool.c
    cap = CAP[group]
    words = 3 * c.fq_limbs * group
    fn = ctx.lib.zkp_msm_g1_var_batch_dev if group == 1 else ctx.lib.zkp_msm_g2_var_batch_dev
    out = np.full((2, words), 0xABABABABABABABAB, dtype=np.uint64)
    xs = (ctypes.c_void_p * 2)(pool.dxy, pool.dxy)
    ss = (ctypes.c_void_p * 2)(pool.dk, pool.dk)
    for bad in ((cap + 1, 8), (8, cap + 1)):
        ns = (ctypes.c_size_t * 2)(*bad)
        assert fn(ctx.h, c.cid, 2, xs, None, ss, ns, 0, ctypes.c_void_p(out.ctypes.data)) == -1
        assert (out == 0xABABABABABABABAB).all()
    ns = (ctypes.c_size_t * 2)(8, 8)
    assert fn(ctx.h, c.cid, 0, None, None, None, None, 0, ctypes.c_void_p(out.ctypes.data)) == 0
    assert (out == 0xABABABABABABABAB).all()
    assert fn(ctx.h, c.cid, 2, xs, None, ss, ns, 0, ctypes.c_void_p(out.ctypes.data)) == 0
    exp = pool.expect([pool.dlog(0, 0, 8)])[0]
    assert _affine(curve, group, out) == [exp, exp]
    got = pool.run(ctx, [pool.entry(0, cap, cap)])
    assert _affine(curve, group, got) == pool.expect([pool.dlog(0, cap, cap)])


def test_two_threads_two_contexts():
    """Two contexts in two threads run different batches concurrently; each gets its own, correct results."""
    curve, group = "bn254", 1
    results, errors = {}, []

    def worker(tid):
        try:
            with Context(0) as cx:
                p = Pool(cx, curve, group, seed=300 + tid)
                try:
                    rnd = random.Random(tid)
                    entries = []
                    for _ in range(24):
                        n = rnd.randrange(1, 3000)
                        entries.append((rnd.randrange(CAP[group] - n), rnd.randrange(CAP[group]), n))
                    exp = p.expect([p.dlog(b, s, n) for b, s, n in entries])
                    for _ in range(3):
                        out = p.run(cx, [p.entry(b, s, n) for b, s, n in entries])
                        assert _affine(curve, group, out) == exp
                    results[tid] = True
                finally:
                    p.free()
        except Exception as e:                        # noqa: BLE001 — reported by the main thread
            errors.append((tid, e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    assert not errors, errors
    assert results == {0: True, 1: True}


@pytest.mark.parametrize("curve,group", CFG)
def test_reproducible(ctx, curve, group, pool):
    """The same batch twice: bit-identical Jacobian limbs (the LDS sort is stable, the reductions run in a fixed order)."""
    rnd = random.Random(3)
    entries = [pool.entry(rnd.randrange(1000), rnd.randrange(1000), n) for n in (0, 5, 700, 4096, 9000)]
    a = pool.run(ctx, entries)
    b = pool.run(ctx, entries)
    assert np.array_equal(a, b)
