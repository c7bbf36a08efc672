"""zkp_fr_product_circuit_dev / zkp_fr_memcheck_circuits_dev / ckb_zkp_amd.spark on the device, bit-exact against
tests/spark_ref.py (Python integers that follow spartan/src/spark.rs, prover.rs and verify.rs)."""
import ctypes
import hashlib

import numpy as np
import pytest

from ckb_zkp_amd import codec, spark
from ckb_zkp_amd.params import get_curve
from tests import spark_ref as ref
from tests.util import TEST_FULL

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xABABABABABABABAB
U32_MAX = 0xFFFFFFFF


def _rand(c, n, seed):
    """n nonzero field elements as integers"""
    rng = np.random.default_rng(seed)
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)      # < 2^(bits - 1) < r
    return [v or 1 for v in codec.limbs_to_ints(k)]


def _m(c, x):
    return codec.fr_to_mont([x], c)[0]


class Circuits:
    """count circuit buffers of 2n - 2 elements side by side in one device buffer, a sentinel element before and after each"""

    def __init__(self, ctx, count, n):
        self.ctx, self.count, self.n = ctx, count, n
        self.host = np.full((count, 2 * n, 4), SENT, dtype=np.uint64)
        self.dev = ctx.to_device(self.host)

    def ptr(self, i):
        return self.dev + 32 * (2 * self.n * i + 1)

    def ptrs(self):
        return [self.ptr(i) for i in range(self.count)]

    def set_leaves(self, c, leaves):
        """leaves: count lists of n integers -> layer 0 of every circuit"""
        for i, lv in enumerate(leaves):
            self.host[i, 1:1 + self.n] = codec.fr_to_mont(lv, c)
        self.ctx.h2d(self.dev, self.host)

    def read(self):
        out = np.zeros_like(self.host)
        self.ctx.d2h(out, self.dev)
        return out

    def expected(self, c, leaves):
        """the whole buffer as the reference fills it, sentinels included, and the roots"""
        exp = np.full_like(self.host, SENT)
        roots = []
        for i, lv in enumerate(leaves):
            circ = ref.construct_product_circuit(lv, c.r)
            exp[i, 1:2 * self.n - 1] = codec.fr_to_mont(ref.flatten(circ), c)
            roots.append(ref.evaluate_product_circuit(circ, c.r))
        return exp, roots

    def free(self):
        self.ctx.dev_free(self.dev)


# ------------------------------------------------------------------------------------------- product circuits
# 2^1 .. 2^13: the root-only case, every value of log2 n mod 3, the hand-over to strided passes above 2^9 (one pass of radix 2, 4, 8
# at 2^10, 2^11, 2^12) and the first length with two strided passes (2^13)
@pytest.mark.parametrize("log_n", range(1, 14))
@pytest.mark.parametrize("curve", CURVES)
def test_product_circuit(ctx, curve, log_n):
    c = get_curve(curve)
    n = 1 << log_n
    for count in (1, 3, 16):
        pool = _rand(c, count * n, 100 * log_n + count)
        leaves = [pool[i * n:(i + 1) * n] for i in range(count)]
        leaves[0][n - 1] = c.r - 1
        if count > 1:
            leaves[1][n // 2] = 0                                  # a zero leaf: every layer above it has a zero, the root is 0
        cs = Circuits(ctx, count, n)
        try:
            cs.set_leaves(c, leaves)
            exp, exp_roots = cs.expected(c, leaves)
            if count > 1:
                assert exp_roots[1] == 0 and exp_roots[0] != 0
            roots = ctx.fr_product_circuit_dev(c, cs.ptrs(), n)
            assert codec.fr_from_mont(roots, c) == exp_roots, count
            got = cs.read()
            assert np.array_equal(got[:, 0], exp[:, 0]) and np.array_equal(got[:, -1], exp[:, -1]), (count, "sentinels")
            assert np.array_equal(got, exp), count
            again = ctx.fr_product_circuit_dev(c, cs.ptrs(), n)
            assert again.tobytes() == roots.tobytes() and cs.read().tobytes() == got.tobytes(), (count, "second call")
        finally:
            cs.free()


# ------------------------------------------------------------------------------------------- hashes + circuits
def _leaf_inputs(c, n, seed):
    """two address arrays, two value arrays, two timestamp arrays with the edge values of a k = 3 instance over m = 2^28 cells"""
    rng = np.random.default_rng(seed)
    m = 1 << 28
    a0 = rng.integers(0, m, size=n, dtype=np.uint32)
    a1 = rng.integers(0, m, size=n, dtype=np.uint32)
    a0[0], a0[-1] = m - 1, 0
    a1[0] = U32_MAX
    t0 = rng.integers(0, 3 * n, size=n, dtype=np.uint32)
    t1 = rng.integers(0, 3 * n, size=n, dtype=np.uint32)
    t0[0], t0[-1] = 0, 3 * n                                       # audit_ts of a cell that every one of the 3 n operations hit
    t1[0], t1[-1] = 3 * (1 << 28), U32_MAX                         # the same at the largest n; the largest uint32 (+ 1 leaves 32 bits)
    v0, v1 = _rand(c, n, seed + 1), _rand(c, n, seed + 2)
    v0[0], v1[0], v1[-1] = c.r - 1, 0, c.r - 1
    return (a0, a1), (v0, v1), (t0, t1)


def _ref_leaves(c, n, addr, val, ts, ts_add, g1, g2):
    a = list(range(n)) if addr is None else [int(x) for x in addr]
    t = [ts_add] * n if ts is None else [int(x) + ts_add for x in ts]
    return [(h - g2) % c.r for h in ref.circuit_hash(a, val, t, g1, c.r)]


# 2^10: the only length whose first launch is the radix-2 instance of the fused leaf pass
@pytest.mark.parametrize("n", [2, 8, 64, 1 << 10, 1 << 11])
@pytest.mark.parametrize("curve", CURVES)
def test_memcheck_circuits(ctx, curve, n):
    c = get_curve(curve)
    r = c.r
    (a0, a1), (v0, v1), (t0, t1) = _leaf_inputs(c, n, 7 * n)
    bufs = [ctx.to_device(x) for x in (a0, a1, codec.fr_to_mont(v0, c), codec.fr_to_mont(v1, c), t0, t1)]
    da0, da1, dv0, dv1, dt0, dt1 = bufs
    # (addr, val, ts, ts_add): host values and device pointers
    entries = [((a0, v0, t0, 0), (da0, dv0, dt0)),
               ((a0, v0, t0, 1), (da0, dv0, dt0)),                 # write = read + 1 on shared inputs
               ((None, v1, None, 0), (None, dv1, None)),           # init: addr = i, ts = 0
               ((None, v1, t1, 0), (None, dv1, dt1)),              # audit: addr = i
               ((a1, v0, None, 1), (da1, dv0, None)),              # NULL ts with + 1
               ((a0, v0, t0, 0), (da0, dv0, dt0)),                 # the first entry again
               ((a1, v1, t1, 1), (da1, dv1, dt1))]                 # + 1 alone, past 32 bits
    count = len(entries)
    rnd = _rand(c, 2, n)
    cs = Circuits(ctx, count, n)
    try:
        for g1, g2 in ((0, 0), (1, r - 1), (r - 1, 1), (rnd[0], rnd[1])):
            cs.ctx.h2d(cs.dev, cs.host)                            # sentinels everywhere
            leaves = [_ref_leaves(c, n, a, v, t, add, g1, g2) for (a, v, t, add), _ in entries]
            exp, exp_roots = cs.expected(c, leaves)
            roots = ctx.fr_memcheck_circuits_dev(c, [d[0] for _, d in entries], [d[1] for _, d in entries], [d[2] for _, d in entries],
                                                 [h[3] for h, _ in entries], cs.ptrs(), n, _m(c, g1), _m(c, g2))
            got = cs.read()
            assert np.array_equal(got[:, 1:1 + n], exp[:, 1:1 + n]), (g1, g2, "leaves")
            assert np.array_equal(got, exp), (g1, g2, "layers and sentinels")
            assert codec.fr_from_mont(roots, c) == exp_roots, (g1, g2)
    finally:
        cs.free()
        for p in bufs:
            ctx.dev_free(p)


# ------------------------------------------------------------------------------------------- argument rules
@pytest.mark.parametrize("curve", CURVES)
def test_errors_leave_everything_untouched(ctx, curve):
    c = get_curve(curve)
    n = 16
    V = ctypes.c_void_p
    cs = Circuits(ctx, 3, n)
    inputs = np.full((4, n, 4), SENT, dtype=np.uint64)             # val, val, addr, ts (the last two read as uint32)
    dev_in = ctx.to_device(inputs)
    val, val2, addr, ts = (dev_in + 32 * n * i for i in range(4))
    roots = np.full((258, 4), SENT, dtype=np.uint64)
    good = _m(c, 5)
    big = np.frombuffer(c.r.to_bytes(32, "little"), dtype=np.uint64).copy()      # r: not reduced
    kp = lambda a: None if a is None else V(a.ctypes.data)        # noqa: E731
    arr = lambda ps: None if ps is None else (V * max(len(ps), 1))(*[p or None for p in ps])   # noqa: E731
    P = cs.ptrs()

    def prod(cu=c.cid, circ=P, n=n, count=None, out=roots):
        return ctx.lib.zkp_fr_product_circuit_dev(ctx.h, cu, len(circ) if count is None else count, arr(circ), n, kp(out))

    base = dict(cu=c.cid, a=[addr, None, addr], v=[val, val, val2], t=[ts, ts, None], add=[0, 1, 1], circ=P, n=n, g1=good, g2=good,
                out=roots)

    def mc(**kw):
        a = dict(base, **kw)
        count = a.get("count", len(a["circ"]) if a["circ"] is not None else 3)
        add = None if a["add"] is None else (ctypes.c_uint32 * max(len(a["add"]), 1))(*a["add"])
        return ctx.lib.zkp_fr_memcheck_circuits_dev(ctx.h, a["cu"], count, arr(a["a"]), arr(a["v"]), arr(a["t"]), add, arr(a["circ"]),
                                                    a["n"], kp(a["g1"]), kp(a["g2"]), kp(a["out"]))
    try:
        for kw in (dict(circ=None, count=3), dict(out=None), dict(circ=[P[0], 0, P[2]]), dict(circ=[P[0], P[1] + 8, P[2]]),   # NULL, misaligned
                   dict(n=0), dict(n=1), dict(n=6), dict(n=24), dict(n=1 << 29),                   # not a power of two in [2, 2^28]
                   dict(circ=[], count=0), dict(circ=[P[0]] * 257),                                # count outside [1, 256]
                   dict(circ=[P[0], P[1], P[0]]), dict(circ=[P[0], P[0] + 32, P[2]]),              # circuits overlap
                   dict(circ=[P[0], P[0] + 32 * (2 * n - 3), P[2]])):
            assert prod(**kw) == -1, kw
            if "count" not in kw and len(kw.get("circ", P)) == 3:          # the same rule through the hash entry point
                assert mc(**kw) == -1, kw
        assert prod(cu=7) == -2 and mc(cu=7) == -2
        for kw in (dict(a=None), dict(v=None), dict(t=None), dict(add=None), dict(g1=None), dict(g2=None),   # NULL arrays
                   dict(v=[val, 0, val2]), dict(v=[val, val + 8, val2]), dict(a=[addr + 2, None, addr]), dict(t=[ts, ts + 1, None]),
                   dict(add=[0, 2, 1]), dict(add=[0, 1, U32_MAX]), dict(g1=big), dict(g2=big),
                   dict(circ=[], a=[], v=[], t=[], add=[], count=0),
                   dict(v=[val, P[2] + 32, val2]), dict(a=[P[1] + 64, None, addr]), dict(t=[ts, ts, P[0] - 4 * n + 4])):   # a circuit overlaps an input
            assert mc(**kw) == -1, kw
        assert np.array_equal(cs.read(), cs.host) and (roots == SENT).all()
        chk = np.zeros_like(inputs)
        ctx.d2h(chk, dev_in)
        assert (chk == SENT).all()
        # good calls: shared and adjacent inputs are fine
        leaves = [_rand(c, n, 900 + i) for i in range(3)]
        cs.set_leaves(c, leaves)
        exp, exp_roots = cs.expected(c, leaves)
        assert prod() == 0
        assert codec.fr_from_mont(roots[:3], c) == exp_roots and (roots[3:] == SENT).all()
        assert np.array_equal(cs.read(), exp)
        ctx.h2d(dev_in, np.zeros_like(inputs))
        assert mc() == 0
        g = 5
        leaves = [_ref_leaves(c, n, a, [0] * n, t, add, g, g) for a, t, add in (([0] * n, [0] * n, 0), (None, [0] * n, 1), ([0] * n, None, 1))]
        exp, exp_roots = cs.expected(c, leaves)
        assert codec.fr_from_mont(roots[:3], c) == exp_roots and np.array_equal(cs.read(), exp)
    finally:
        cs.free()
        ctx.dev_free(dev_in)


# ------------------------------------------------------------------------------------------- driver
def _callbacks(c, tag=b""):
    """deterministic stand-ins for the transcript: a counter plus whatever the reference would have absorbed"""
    state = {"n": 0}

    def h(*parts):
        state["n"] += 1
        data = tag + state["n"].to_bytes(4, "little") + b"".join(int(v).to_bytes(32, "little") for v in parts)
        return int.from_bytes(hashlib.sha256(data).digest(), "little") % c.r

    return (lambda count: [h(count, i) for i in range(count)], lambda coeffs: h(*coeffs),
            lambda left, right, dotp: h(*left, *right, *([v for t in dotp for v in t] if dotp else [])))


@pytest.mark.parametrize("with_dotp", [False, True])
@pytest.mark.parametrize("n,m", [(16, 4), (8, 64), (256, 256)])
@pytest.mark.parametrize("curve", CURVES)
def test_memory_checking_and_eval_prover(ctx, curve, n, m, with_dotp):
    c = get_curve(curve)
    r = c.r
    k = 3
    rng = np.random.default_rng(n + m)
    addrs = [rng.integers(0, m, size=n, dtype=np.uint32) for _ in range(k)]
    addrs[0][0], addrs[-1][-1] = m - 1, 0
    mem = _rand(c, m, n * m)
    full = [_rand(c, n, n * m + 1 + i) for i in range(3)]           # row, col, val of the dot-product circuits
    gamma = tuple(_rand(c, 2, n * m + 9))
    read_ts, audit_ts = spark.memory_in_the_head(addrs, m)
    exp_read, exp_audit = ref.memory_in_the_head([a.tolist() for a in addrs], m)
    assert [t.tolist() for t in read_ts] == exp_read and audit_ts.tolist() == exp_audit
    e_ints = [[mem[a] for a in ad.tolist()] for ad in addrs]
    exp_layer = ref.memory_checking([a.tolist() for a in addrs], mem, exp_read, exp_audit, e_ints, gamma, r)
    exp_ops = [x for pair in zip(exp_layer["read"], exp_layer["write"]) for x in pair]
    bufs = []

    def up(a):
        bufs.append(ctx.to_device(np.ascontiguousarray(a)))
        return bufs[-1]

    layer = None
    try:
        d_mem, d_audit = up(codec.fr_to_mont(mem, c)), up(audit_ts)
        d_addrs, d_ts = [up(a) for a in addrs], [up(t) for t in read_ts]
        d_e = []
        for da in d_addrs:                                           # e_k = mem[addrs_k] with the existing gather
            bufs.append(ctx.dev_alloc(32 * n))
            ctx.fr_gather(d_mem, da, n, bufs[-1])
            d_e.append(bufs[-1])
        d_full = [up(codec.fr_to_mont(t, c)) for t in full]
        layer = spark.memory_checking(ctx, c, d_addrs, d_mem, d_ts, d_audit, d_e, n, m, gamma)
        ev = lambda circ: ref.evaluate_product_circuit(circ, r)   # noqa: E731
        assert layer.roots == dict(init=ev(exp_layer["init"]), audit=ev(exp_layer["audit"]), read=[ev(x) for x in exp_layer["read"]],
                                   write=[ev(x) for x in exp_layer["write"]])
        h = n // 2
        dotp = [tuple(p for p in d_full), tuple(p + 32 * h for p in d_full)] if with_dotp else []
        dotp_ints = [tuple(t[:h] for t in full), tuple(t[h:] for t in full)] if with_dotp else []
        got = spark.product_circuit_eval_prover(ctx, c, layer.ops(), n, dotp, *_callbacks(c))
        assert got == ref.product_circuit_eval_prover(exp_ops, dotp_ints, *_callbacks(c), r)
        layers, claim_dotp, rands = got
        roots = [x for pair in zip(layer.roots["read"], layer.roots["write"]) for x in pair]
        sums = [ref.evaluate_dot_product_circuit(*t, r) for t in dotp_ints]
        claims, claims_dotp, v_rands = ref.product_circuit_eval_verify((layers, claim_dotp), roots, sums, n, *_callbacks(c), r)
        assert v_rands == rands and len(claims_dotp) == (3 if with_dotp else 0)
        # the memory side: init and audit over m leaves
        got = spark.product_circuit_eval_prover(ctx, c, layer.mem(), m, [], *_callbacks(c, b"m"))
        assert got == ref.product_circuit_eval_prover([exp_layer["init"], exp_layer["audit"]], [], *_callbacks(c, b"m"), r)
        ref.product_circuit_eval_verify(got[:2], [layer.roots["init"], layer.roots["audit"]], [], m, *_callbacks(c, b"m"), r)
        if not with_dotp:
            ctx.h2d(d_e[1] + 32 * (n - 1), _m(c, (e_ints[1][n - 1] + 1) % r))      # one changed e value
            with pytest.raises(ValueError):
                spark.memory_checking(ctx, c, d_addrs, d_mem, d_ts, d_audit, d_e, n, m, gamma)
    finally:
        if layer is not None:
            layer.free(ctx)
        for p in bufs:
            ctx.dev_free(p)


def test_whole_circuit_full_size(ctx):
    """the read and write circuits of one list of 2^18 operations (ZKP_TEST_FULL=0: 2^14) through the hash entry point: every
    element of both buffers"""
    c = get_curve("bn254")
    r = c.r
    n = 1 << (18 if TEST_FULL else 14)
    m = 1 << 20
    rng = np.random.default_rng(18)
    addr = rng.integers(0, m, size=n, dtype=np.uint32)
    ts = rng.integers(0, 3 * n, size=n, dtype=np.uint32)
    val_words = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    val_words[:, 3] &= np.uint64((1 << 60) - 1)                    # any words below r are some element's Montgomery form
    val = codec.fr_from_mont(val_words, c)
    g1, g2 = _rand(c, 2, 19)
    bufs = [ctx.to_device(addr), ctx.to_device(val_words), ctx.to_device(ts)]
    cs = Circuits(ctx, 2, n)
    try:
        roots = ctx.fr_memcheck_circuits_dev(c, [bufs[0]] * 2, [bufs[1]] * 2, [bufs[2]] * 2, [0, 1], cs.ptrs(), n, _m(c, g1), _m(c, g2))
        exp, exp_roots = cs.expected(c, [_ref_leaves(c, n, addr.tolist(), val, ts.tolist(), add, g1, g2) for add in (0, 1)])
        assert codec.fr_from_mont(roots, c) == exp_roots
        assert np.array_equal(cs.read(), exp)
    finally:
        cs.free()
        for p in bufs:
            ctx.dev_free(p)
