"""zkp_gkr_layer_* / zkp_fr_gkr_eval_layer_dev / zkp_fr_gkr_tables_dev / zkp_fr_gkr_round_dev / ckb_zkp_amd.gkr on the device,
bit-exact against tests/gkr_ref.py (Python integers that follow libra/src/circuit.rs, evaluate.rs, sumcheck.rs and
libra_linear_gkr.rs).  Every output buffer starts as sentinels with one sentinel element before and after it, and whole buffers are
compared.

The second-stage loops take their second trip in test_tables_one_segment_of_more_chunks_than_threads (gkr_long_kernel: one node of
GKR_THREADS GKR_CHUNK + 1 gates; 0.9 s a curve on an MI355X, the Python tables over 2^20 gates) and
test_round_more_workgroups_than_final_threads (gkr_final_kernel: 2 GKR_THREADS workgroups; under 0.1 s a case)."""
import ctypes

import numpy as np
import pytest

from ckb_zkp_amd import codec, gkr
from ckb_zkp_amd.gkr import GKR_CHUNK, GKR_LONG
from ckb_zkp_amd.params import get_curve
from tests import gkr_ref as ref
from tests.gkr_cases import callbacks, load_mini, rand_fr, random_layers
from tests.sumcheck_ref import combine_with_r
from tests.util import csrc_constant, periodic_bind, periodic_round_sums

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xABABABABABABABAB
V = ctypes.c_void_p
GKR_THREADS = csrc_constant("gkr.hip", "GKR_THREADS")      # threads of gkr_long_kernel and gkr_final_kernel: their loops' stride
PERIOD = 1021                                               # long tables repeat a block of this (prime) length


class Bufs:
    """count buffers of n Fr side by side in one device allocation, a sentinel element before and after each"""

    def __init__(self, ctx, count, n):
        self.ctx, self.count, self.n = ctx, count, n
        self.host = np.full((count, n + 2, 4), SENT, dtype=np.uint64)
        self.dev = ctx.to_device(self.host)

    def ptr(self, i):
        return self.dev + 32 * ((self.n + 2) * i + 1)

    def ptrs(self):
        return [self.ptr(i) for i in range(self.count)]

    def fill(self, c, tables):
        """tables: count lists of n integers (None: sentinels)"""
        self.host[:] = SENT
        for i, t in enumerate(tables):
            if t is not None:
                self.host[i, 1:-1] = codec.fr_to_mont(t, c)
        self.ctx.h2d(self.dev, self.host)

    def read(self):
        out = np.zeros_like(self.host)
        self.ctx.d2h(out, self.dev)
        return out

    def expected(self, c, tables):
        exp = np.full_like(self.host, SENT)
        for i, t in enumerate(tables):
            if t is not None:
                exp[i, 1:-1] = codec.fr_to_mont(t, c)
        return exp

    def free(self):
        self.ctx.dev_free(self.dev)


def _upload(ctx, gates, log_in):
    a = np.asarray(gates, dtype=np.int64).reshape(-1, 3)
    return ctx.gkr_layer_upload(a[:, 0], a[:, 1], a[:, 2], log_in)


def _values(c, n, seed):
    v = rand_fr(c.r, n, seed)
    v[0] = 0
    v[-1] = c.r - 1
    if n > 2:
        v[1] = c.r - 1
    return v


# ------------------------------------------------------------------------------------------- layer evaluation
@pytest.mark.parametrize("n_gates", [1, 2, 3, 255, 256, 257, 1000])
@pytest.mark.parametrize("curve", CURVES)
def test_eval_layer(ctx, curve, n_gates):
    c = get_curve(curve)
    log_in = 5
    nodes = 1 << log_in
    below = _values(c, nodes, n_gates)                            # operands 0 and r - 1 at nodes 0, 1 and 31
    log_out = (n_gates - 1).bit_length()
    d_in = ctx.to_device(codec.fr_to_mont(below, c))
    out = Bufs(ctx, 1, 1 << log_out)
    try:
        for mode in ("add", "mul", "mixed"):
            gates = random_layers([n_gates], nodes, 10 * n_gates + len(mode))[0]       # indices 0 and 31, left == right
            gates = [({"add": 0, "mul": 1}.get(mode, o), a, b) for o, a, b in gates]
            if n_gates >= 3:
                gates[2] = (gates[2][0], 1, 31)                    # (r - 1) op (r - 1)
            layer = _upload(ctx, gates, log_in)
            try:
                info = ctx.gkr_layer_info(layer)
                assert (info["n_gates"], info["log_out"], info["log_in"]) == (n_gates, log_out, log_in)
                assert info["n_mul"] == sum(g[0] for g in gates)
                out.fill(c, [None])
                ctx.fr_gkr_eval_layer_dev(c, layer, d_in, out.ptr(0))
                exp = ref.eval_layer(gates, below, c.r)
                assert len(exp) == 1 << log_out and all(v == 0 for v in exp[n_gates:])   # the padding zeros
                assert np.array_equal(out.read(), out.expected(c, [exp])), mode
            finally:
                ctx.gkr_layer_free(layer)
    finally:
        out.free()
        ctx.dev_free(d_in)


# ------------------------------------------------------------------------------------------- bookkeeping tables
def _check_tables(ctx, c, gates, log_in, seed, long_left, long_right):
    """both phases of one layer against eval_hg / eval_fgu; returns the layer's info"""
    nodes, n_gates = 1 << log_in, len(gates)
    log_out = (n_gates - 1).bit_length()
    g_vec, w_vec = _values(c, 1 << log_out, seed), _values(c, nodes, seed + 1)
    ref_gates = [(g, o, a, b) for g, (o, a, b) in enumerate(gates)]
    layer = _upload(ctx, gates, log_in)
    d_in = ctx.to_device(np.concatenate([codec.fr_to_mont(g_vec, c), codec.fr_to_mont(w_vec, c)]))
    d_g, d_w = d_in, d_in + 32 * len(g_vec)
    out = Bufs(ctx, 3, nodes)
    try:
        info = ctx.gkr_layer_info(layer)
        assert (info["n_gates"], info["log_out"], info["log_in"]) == (n_gates, log_out, log_in)
        fan = lambda k: max(np.bincount([g[k] for g in gates], minlength=nodes))       # noqa: E731
        assert (info["max_fan_left"], info["max_fan_right"]) == (fan(1), fan(2))
        assert (info["long_left"], info["long_right"]) == (long_left, long_right)        # which path runs
        for phase in (1, 2):
            exp = ref.eval_hg(g_vec, w_vec, ref_gates, log_in, c.r) if phase == 1 else ref.eval_fgu(g_vec, w_vec, ref_gates, log_in, c.r)
            exp = list(exp) + [None] * (3 - len(exp))
            out.fill(c, [None] * 3)
            ctx.fr_gkr_tables_dev(c, layer, phase, d_g, d_w, out.ptrs()[:4 - phase])
            got = out.read()
            assert np.array_equal(got, out.expected(c, exp)), phase
            ctx.fr_gkr_tables_dev(c, layer, phase, d_g, d_w, out.ptrs()[:4 - phase])
            assert out.read().tobytes() == got.tobytes(), (phase, "second call")
        return info
    finally:
        out.free()
        ctx.dev_free(d_in)
        ctx.gkr_layer_free(layer)


@pytest.mark.parametrize("log_in", range(1, 12))
@pytest.mark.parametrize("curve", CURVES)
def test_tables_random_wiring(ctx, curve, log_in):
    c = get_curve(curve)
    nodes = 1 << log_in
    n_gates = 3 * nodes // 2 + 1
    rng = np.random.default_rng(log_in)
    left, right = rng.integers(0, nodes, size=n_gates), rng.integers(0, nodes, size=n_gates)
    left[left == 1] = 0                                            # node 1 has no gates on the left,
    right[right == nodes - 2] = nodes - 1                          # node 2^log_in - 2 none on the right
    left[0], right[0], left[1], right[1] = nodes - 1, 0, 0, nodes - 1
    op = rng.integers(0, 2, size=n_gates)
    op[0], op[1] = 0, 1
    gates = [(int(o), int(a), int(b)) for o, a, b in zip(op, left, right)]
    info = _check_tables(ctx, c, gates, log_in, 100 + log_in, 0, 0)
    assert info["max_fan_left"] <= GKR_LONG and 0 < info["n_mul"] < n_gates


@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("curve", CURVES)
def test_tables_only_one_kind_of_gate(ctx, curve, op):
    c = get_curve(curve)
    gates = [(op, a, b) for _, a, b in random_layers([300], 64, 3 + op)[0]]
    info = _check_tables(ctx, c, gates, 6, 40 + op, 0, 0)
    assert info["n_mul"] == op * 300


def _hot_gates(nodes, fans, seed):
    """fans[i] gates read node 3 + 2 i on the left (right wire random), as many read it on the right (left wire random);
    100 more avoid those nodes"""
    rng = np.random.default_rng(seed)
    hot = [3 + 2 * i for i in range(len(fans))]
    cold = [v for v in range(nodes) if v not in hot]
    pick = lambda k: rng.choice(cold, size=k)                      # noqa: E731
    left = np.concatenate([np.full(f, h) for f, h in zip(fans, hot)] + [pick(sum(fans)), pick(100)])
    right = np.concatenate([pick(sum(fans))] + [np.full(f, h) for f, h in zip(fans, hot)] + [pick(100)])
    op = rng.integers(0, 2, size=len(left))
    order = rng.permutation(len(left))                             # the hot gates are spread over the gate list
    return [(int(op[i]), int(left[i]), int(right[i])) for i in order]


# the last fan-out handled by one thread, the first cut into chunks (one chunk), a full chunk, two chunks, four chunks
@pytest.mark.parametrize("fan", [GKR_LONG - 1, GKR_LONG, GKR_LONG + 1, GKR_CHUNK, GKR_CHUNK + 1, 3 * GKR_CHUNK + 1])
@pytest.mark.parametrize("curve", CURVES)
def test_tables_one_hot_node(ctx, curve, fan):
    c = get_curve(curve)
    n_long = 1 if fan > GKR_LONG else 0
    info = _check_tables(ctx, c, _hot_gates(256, [fan], fan), 8, fan, n_long, n_long)
    assert info["max_fan_left"] == info["max_fan_right"] == fan


@pytest.mark.parametrize("curve", CURVES)
def test_tables_two_long_nodes(ctx, curve):
    c = get_curve(curve)
    _check_tables(ctx, c, _hot_gates(256, [GKR_LONG + 1, GKR_CHUNK + 5], 77), 8, 78, 2, 2)


@pytest.mark.parametrize("curve", CURVES)
def test_tables_one_segment_of_more_chunks_than_threads(ctx, curve):
    """GKR_THREADS GKR_CHUNK + 1 gates, all of them (op, 0, 1): node 0 on the left and node 1 on the right each hold one segment of
    GKR_THREADS + 1 chunks, so thread 0 of gkr_long_kernel adds a second partial (the chunk of one gate) in both phases.  G repeats
    PERIOD values, the ops repeat a block of 7; the tables are eval_hg / eval_fgu over the whole gate list."""
    c = get_curve(curve)
    r = c.r
    log_in, nodes = 1, 2
    n_gates = GKR_THREADS * GKR_CHUNK + 1
    assert -(-n_gates // GKR_CHUNK) == GKR_THREADS + 1 and n_gates > GKR_LONG
    log_out = (n_gates - 1).bit_length()
    op = np.resize(np.array([0, 1, 1, 0, 1, 0, 0], dtype=np.uint8), n_gates)
    left, right = np.zeros(n_gates, dtype=np.uint32), np.ones(n_gates, dtype=np.uint32)
    base = _values(c, PERIOD, 7)
    idx = np.arange(1 << log_out) % PERIOD
    g_vec, w_vec = [base[i] for i in idx.tolist()], [r - 1, rand_fr(r, 1, 8)[0]]
    ref_gates = list(zip(range(n_gates), op.tolist(), left.tolist(), right.tolist()))
    layer = ctx.gkr_layer_upload(op, left, right, log_in)
    g_words = codec.fr_to_mont(base, c)[idx]
    d_in = ctx.to_device(np.concatenate([g_words, codec.fr_to_mont(w_vec, c)]))
    d_g, d_w = d_in, d_in + 32 * len(g_vec)
    out = Bufs(ctx, 3, nodes)
    try:
        info = ctx.gkr_layer_info(layer)
        assert (info["n_gates"], info["log_out"], info["log_in"], info["n_mul"]) == (n_gates, log_out, log_in, int(op.sum()))
        assert (info["max_fan_left"], info["max_fan_right"], info["long_left"], info["long_right"]) == (n_gates, n_gates, 1, 1)
        for phase in (1, 2):
            exp = ref.eval_hg(g_vec, w_vec, ref_gates, log_in, r) if phase == 1 else ref.eval_fgu(g_vec, w_vec, ref_gates, log_in, r)
            assert all(t[phase - 1] != 0 and t[2 - phase] == 0 for t in exp)      # the long node's slot; the other node has no gates
            exp = list(exp) + [None] * (3 - len(exp))
            out.fill(c, [None] * 3)
            ctx.fr_gkr_tables_dev(c, layer, phase, d_g, d_w, out.ptrs()[:4 - phase])
            assert np.array_equal(out.read(), out.expected(c, exp)), phase
        got_in = np.zeros((len(g_vec) + 2, 4), dtype=np.uint64)
        ctx.d2h(got_in, d_in)
        assert np.array_equal(got_in[:-2], g_words), "G changed"
    finally:
        out.free()
        ctx.dev_free(d_in)
        ctx.gkr_layer_free(layer)


@pytest.mark.parametrize("curve", CURVES)
def test_tables_errors_leave_everything_untouched(ctx, curve):
    c = get_curve(curve)
    log_in, nodes = 4, 16
    gates = random_layers([16], nodes, 9)[0]
    layer = _upload(ctx, gates, log_in)
    inp = Bufs(ctx, 2, nodes)
    out = Bufs(ctx, 3, nodes)
    try:
        inp.fill(c, [_values(c, nodes, 1), _values(c, nodes, 2)])
        out.fill(c, [None] * 3)
        g, w = inp.ptrs()
        o = out.ptrs()

        def call(phase=1, g=g, w=w, outs=(o[0], o[1], o[2]), layer=layer, cu=c.cid):
            arr = None if outs is None else (V * 3)(*[p or None for p in outs])
            return ctx.lib.zkp_fr_gkr_tables_dev(ctx.h, cu, V(layer), phase, V(g), V(w), arr)

        for kw in (dict(phase=0), dict(phase=3), dict(g=None), dict(w=None), dict(outs=None), dict(layer=None),
                   dict(outs=(o[0], o[1], None)), dict(phase=2, outs=(o[0], None, None)), dict(phase=2),       # NULL outputs / out[2] in phase 2
                   dict(g=g + 8), dict(w=w + 8), dict(outs=(o[0], o[1] + 8, o[2])),                              # misaligned
                   dict(outs=(o[0], o[0], o[2])), dict(outs=(o[0], o[0] + 32, o[2])), dict(outs=(o[0], o[1], o[1] + 32 * (nodes - 1))),
                   dict(outs=(g, o[1], o[2])), dict(outs=(o[0], w + 32 * (nodes - 1), o[2])), dict(phase=2, outs=(o[0], g - 32, None))):
            assert call(**kw) == -1, kw
        assert call(cu=7) == -2
        assert np.array_equal(out.read(), out.host) and np.array_equal(inp.read(), inp.host)
        assert call() == 0 and call(phase=2, outs=(o[0], o[1], None)) == 0
        # eval layer: output over its input, misaligned, NULL
        ev = lambda i, p: ctx.lib.zkp_fr_gkr_eval_layer_dev(ctx.h, c.cid, V(layer), V(i), V(p))    # noqa: E731
        before = out.read()
        assert ev(w, w) == -1 and ev(w, w + 32 * (nodes - 1)) == -1 and ev(w, o[0] + 8) == -1 and ev(w + 8, o[0]) == -1
        assert ev(None, o[0]) == -1 and ev(w, None) == -1
        assert np.array_equal(out.read(), before) and np.array_equal(inp.read(), inp.host)
    finally:
        out.free()
        inp.free()
        ctx.gkr_layer_free(layer)


def test_upload_rules(ctx):
    p = lambda a: V(a.ctypes.data)                                 # noqa: E731
    handle = V()

    def up(op, left, right, n=None, log_in=1):
        op, left, right = np.array(op, dtype=np.uint8), np.array(left, dtype=np.uint32), np.array(right, dtype=np.uint32)
        return ctx.lib.zkp_gkr_layer_upload(ctx.h, p(op), p(left), p(right), len(op) if n is None else n, log_in, ctypes.byref(handle))

    assert up([0, 2], [0, 1], [1, 0]) == -1                        # IllegalOperator
    assert up([0, 1], [0, 2], [1, 0]) == -1 and up([0, 1], [0, 1], [1, 2]) == -1      # IllegalNode
    assert up([0, 1], [0, 1], [1, 0], n=0) == -1 and up([0, 1], [0, 1], [1, 0], log_in=29) == -1
    assert up([0], [1], [1], log_in=0) == -1
    assert handle.value is None
    assert up([0, 1], [0, 1], [1, 0]) == 0 and handle.value
    info = ctx.gkr_layer_info(handle.value)
    assert list(info.values()) == [2, 1, 1, 1, 1, 1, 0, 0]
    ctx.gkr_layer_free(handle.value)
    assert up([1], [0], [0], log_in=0) == 0                        # one gate over a one-gate layer
    assert list(ctx.gkr_layer_info(handle.value).values()) == [1, 0, 0, 1, 1, 1, 0, 0]
    ctx.gkr_layer_free(handle.value)


# ------------------------------------------------------------------------------------------- rounds
# 2: the shortest table that can be evaluated (no bind); 4: the shortest that can be bound and evaluated; 512 / 1024: one workgroup
# without / with a bind; 1024 / 2048: two workgroups; 4096: more
@pytest.mark.parametrize("length", [2, 4, 8, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("phase", [1, 2])
@pytest.mark.parametrize("curve", CURVES)
def test_round(ctx, curve, phase, length):
    c = get_curve(curve)
    r = c.r
    nt = 5 - phase
    tables = [_values(c, length, 10 * length + phase + i) for i in range(nt)]
    x = rand_fr(r, 1, length)[0]
    fus = [None] if phase == 1 else [0, 1, r - 1, rand_fr(r, 1, length + 1)[0]]
    m = lambda v: None if v is None else codec.fr_mont(v, c)      # noqa: E731
    ints = lambda ev: tuple(codec.fr_from_mont(ev, c))            # noqa: E731
    bufs = Bufs(ctx, nt, length)
    try:
        bufs.fill(c, tables)
        for fu in fus:                                             # evaluate only: nothing changes
            assert ints(ctx.fr_gkr_round_dev(c, phase, bufs.ptrs(), length, fu=m(fu))) == ref.round_evals(phase, tables, fu, r), fu
        assert np.array_equal(bufs.read(), bufs.host)
        half = length // 2
        bound = [combine_with_r(t, x, r) for t in tables]
        exp = bufs.expected(c, [b + t[half:] for b, t in zip(bound, tables)])            # the upper half untouched
        if half >= 2:                                              # bind and evaluate
            for fu in fus:
                bufs.fill(c, tables)
                got = ctx.fr_gkr_round_dev(c, phase, bufs.ptrs(), length, fu=m(fu), bind=m(x))
                assert ints(got) == ref.round_evals(phase, bound, fu, r), fu
                assert np.array_equal(bufs.read(), exp), fu
        bufs.fill(c, tables)                                       # bind only
        assert ctx.fr_gkr_round_dev(c, phase, bufs.ptrs(), length, fu=m(fus[-1]), bind=m(x), want_evals=False) is None
        assert np.array_equal(bufs.read(), exp)
        for edge in (0, 1, r - 1):                                 # the challenge itself at its edges
            bufs.fill(c, tables)
            ctx.fr_gkr_round_dev(c, phase, bufs.ptrs(), length, fu=m(fus[-1]), bind=m(edge), want_evals=False)
            assert np.array_equal(bufs.read(), bufs.expected(c, [combine_with_r(t, edge, r) + t[half:] for t in tables])), edge
    finally:
        bufs.free()


@pytest.mark.parametrize("bind", [False, True])
@pytest.mark.parametrize("phase", [1, 2])
@pytest.mark.parametrize("curve", CURVES)
def test_round_more_workgroups_than_final_threads(ctx, curve, phase, bind):
    """2^18 elements without a bind, 2^19 with one: h = 2^17 columns, 2 GKR_THREADS workgroups, the shortest tables at which every
    thread of gkr_final_kernel adds a second partial.  The tables repeat PERIOD values each, so the sums are formed per residue
    (tests/util.periodic_round_sums over ref.round_evals) and the bound halves repeat periodic_bind's block."""
    c = get_curve(curve)
    r = c.r
    nt = 5 - phase
    length = 1 << (19 if bind else 18)
    h = length // (4 if bind else 2)
    assert GKR_THREADS < h // GKR_THREADS <= 2 * GKR_THREADS and (h // 2) // GKR_THREADS <= GKR_THREADS
    bases = [_values(c, PERIOD, 1000 * phase + 10 * bind + i) for i in range(nt)]
    fu = None if phase == 1 else rand_fr(r, 1, 91)[0]
    assert fu not in (0, 1)
    x = rand_fr(r, 1, 92)[0]
    m = lambda v: None if v is None else codec.fr_mont(v, c)      # noqa: E731
    idx = np.arange(length) % PERIOD
    evals = lambda t: ref.round_evals(phase, t, fu, r)            # noqa: E731
    bufs = Bufs(ctx, nt, length)
    try:
        for i, b in enumerate(bases):
            bufs.host[i, 1:-1] = codec.fr_to_mont(b, c)[idx]
        ctx.h2d(bufs.dev, bufs.host)
        exp = bufs.host.copy()
        if bind:
            bases = [periodic_bind(b, length // 2, x, r) for b in bases]
            for i, b in enumerate(bases):
                exp[i, 1:1 + length // 2] = codec.fr_to_mont(b, c)[idx[:length // 2]]       # the upper half untouched
        got = ctx.fr_gkr_round_dev(c, phase, bufs.ptrs(), length, fu=m(fu), bind=m(x) if bind else None)
        assert tuple(codec.fr_from_mont(got, c)) == periodic_round_sums(evals, bases, h, r)
        assert np.array_equal(bufs.read(), exp)
    finally:
        bufs.free()


@pytest.mark.parametrize("curve", CURVES)
def test_round_errors_leave_everything_untouched(ctx, curve):
    c = get_curve(curve)
    length = 16
    bufs = Bufs(ctx, 4, length)
    good = codec.fr_mont(5, c)
    big = np.frombuffer(c.r.to_bytes(32, "little"), dtype=np.uint64).copy()             # r: not reduced
    out = np.full((2, 4), SENT, dtype=np.uint64)
    kp = lambda a: None if a is None else V(a.ctypes.data)        # noqa: E731
    P = bufs.ptrs()
    try:
        bufs.fill(c, [_values(c, length, i) for i in range(4)])

        def call(phase=1, tabs=P, length=length, fu=good, bind=good, ev=out, cu=c.cid):
            arr = None if tabs is None else (V * 4)(*[p or None for p in list(tabs) + [None] * (4 - len(tabs))])
            return ctx.lib.zkp_fr_gkr_round_dev(ctx.h, cu, phase, arr, length, kp(fu), kp(bind), kp(ev))

        for kw in (dict(phase=0), dict(phase=3), dict(phase=-1), dict(tabs=None), dict(bind=None, ev=None),
                   dict(bind=big), dict(phase=2, fu=big), dict(phase=2, fu=None), dict(phase=2, tabs=[P[0], P[1], None]),
                   dict(tabs=[P[0], P[1], None, P[3]]), dict(tabs=[P[0], P[1] + 8, P[2], P[3]]), dict(phase=2, tabs=[P[0] + 4, P[1], P[2]]),
                   dict(tabs=[P[0], P[1], P[0], P[3]]), dict(tabs=[P[0], P[0] + 32 * (length - 1), P[2], P[3]]),
                   dict(length=0), dict(length=12), dict(length=1 << 29), dict(length=1, bind=None), dict(length=2), dict(length=1)):
            assert call(**kw) == -1, kw
        assert call(cu=7) == -2
        assert np.array_equal(bufs.read(), bufs.host) and (out == SENT).all()
        assert call() == 0 and call(phase=2, tabs=P[:3]) == 0 and call(phase=1, fu=None) == 0 and call(phase=2, tabs=P[:3], fu=None, ev=None) == 0
        assert call(length=1, ev=None) == -1 and call(length=2, ev=None) == 0
    finally:
        bufs.free()


# ------------------------------------------------------------------------------------------- whole prover
def _mini():
    _, layers_raw, inputs, witnesses = load_mini()
    return layers_raw, inputs, witnesses


def _random(widths, below, seed, hot=None):
    return lambda r: (random_layers(widths, 2 * below, seed, hot), rand_fr(r, below - 1, seed + 1), rand_fr(r, below, seed + 2))


CASES = {
    "mini": lambda r: _mini(),
    "2-4-8": _random([2, 4, 8], 2, 1),                                           # depth 4
    "one-gate-middle": _random([16, 1, 2, 4], 8, 2),                             # depth 5, zero rounds below the 2-gate layer
    "output-of-3": _random([64, 32, 32, 3], 4, 3),                               # depth 5, a non-power-of-two output layer
    "hot-wire": _random([1024, 512, 5], 32, 4, hot=(1, 7, 0.7)),                 # depth 4, 2^10 wide, ~360 gates on one wire: long segments
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("curve", CURVES)
def test_whole_prover(ctx, curve, case):
    c = get_curve(curve)
    r = c.r
    layers_raw, inputs, aux = CASES[case](r)
    rc = ref.Circuit(len(inputs), len(aux), layers_raw)
    gu = rand_fr(r, rc.layers[-1].bit_size, 5)
    exp_proofs, exp_out, exp_evals, exp_ru, exp_rv = ref.prover(rc, inputs, aux, gu, *callbacks(r), r)
    circuit = gkr.Circuit(ctx, len(inputs), len(aux), layers_raw)
    evals = None
    try:
        assert circuit.counts == [l.gates_count for l in rc.layers] and circuit.bit_sizes == [l.bit_size for l in rc.layers]
        if case == "hot-wire":
            assert circuit.info(2)["long_left"] >= 1 and circuit.info(2)["long_right"] >= 1
        evals = gkr.evaluate(circuit, c, inputs, aux)
        assert [gkr.read_layer(circuit, c, evals, d) for d in range(circuit.depth)] == exp_evals
        result_u = gkr.eval_output(circuit, c, evals, gu)
        assert result_u == ref.eval_output(exp_out, rc.layers[-1].bit_size, gu, r)
        proofs, ru, rv = gkr.prove_layers(circuit, c, evals, gu, result_u, *callbacks(r))
        assert proofs == exp_proofs and (ru, rv) == (exp_ru, exp_rv)           # every polynomial, challenge and final value
        assert ref.verify(rc, proofs, exp_out, exp_evals[0], gu, *callbacks(r), r)
    finally:
        if evals is not None:
            gkr.free_evals(circuit, evals)
        circuit.free()


def test_driver_rules(ctx):
    r = get_curve("bn254").r
    with pytest.raises(ValueError, match="IllegalOperator"):
        gkr.Circuit(ctx, 2, 2, [[(2, 0, 1)]])
    with pytest.raises(ValueError, match="IllegalNode"):
        gkr.Circuit(ctx, 2, 2, [[(0, 0, 1), (1, 1, 2)], [(0, 0, 2)]])           # the layer below has two gates
    circuit = gkr.Circuit(ctx, 2, 2, [[(0, 0, 1), (1, 1, 2), (1, 3, 3)], [(0, 0, 2)]])   # three gates feed a layer
    evals = gkr.evaluate(circuit, "bn254", [1, 2], [3, 4])
    try:
        with pytest.raises(ValueError, match="power-of-two"):
            gkr.prove_layers(circuit, "bn254", evals, [], 0, *callbacks(r))
    finally:
        gkr.free_evals(circuit, evals)
        circuit.free()
