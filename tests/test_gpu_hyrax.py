"""zkp_fr_gkr_eval_layer_batch_dev / zkp_fr_gkr_dp_round_dev / ckb_zkp_amd.hyrax on the device, bit-exact against tests/hyrax_ref.py
(Python integers that follow hyrax/src/zk_sumcheck_proof.rs, hyrax_proof.rs, evaluate.rs and circuit.rs).  Every buffer the device
may write starts with one sentinel element before and after it, whole buffers are compared and the inputs are read again.
test_rounds_more_workgroups_than_sum_threads (HYRAX_THREADS + 1 workgroups under fr_sum_partials) takes under 0.1 s a case on an
MI355X."""
import ctypes

import numpy as np
import pytest

from ckb_zkp_amd import codec, gkr, hyrax
from ckb_zkp_amd.gkr import GKR_LONG
from ckb_zkp_amd.hyrax import HYRAX_CHUNK, HYRAX_THREADS
from ckb_zkp_amd.params import get_curve
from tests import gkr_ref, hyrax_ref as ref
from tests.gkr_cases import rand_fr, random_layers
from tests.hyrax_cases import assignments, callbacks, load_golden, points
from tests.test_gpu_gkr import SENT, Bufs, _upload, _values

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
V = ctypes.c_void_p


def _rows(c, rows, n, seed):
    """rows x n values with 0 and r - 1 among the operands"""
    flat = _values(c, rows * n, seed)
    return [flat[i * n:(i + 1) * n] for i in range(rows)]


def _flat(rows):
    return [v for row in rows for v in row]


# ------------------------------------------------------------------------------------------- layer evaluation over n copies
# n: one copy, two, one wavefront, one workgroup; gates: one, a count that is no power of two (zero rows), more rows than a workgroup
@pytest.mark.parametrize("n", [1, 2, 64, 256])
@pytest.mark.parametrize("n_gates", [1, 3, 5, 300])
@pytest.mark.parametrize("curve", CURVES)
def test_eval_layer_batch(ctx, curve, n_gates, n):
    c = get_curve(curve)
    log_in = 3
    nodes = 1 << log_in
    below = _rows(c, nodes, n, n_gates + n)
    log_out = (n_gates - 1).bit_length()
    inp = Bufs(ctx, 1, nodes * n)
    out = Bufs(ctx, 1, n << log_out)
    try:
        inp.fill(c, [_flat(below)])
        for mode in ("add", "mul", "mixed"):
            gates = random_layers([n_gates], nodes, 10 * n_gates + len(mode))[0]       # node 0 and the last node, left == right
            gates = [({"add": 0, "mul": 1}.get(mode, o), a, b) for o, a, b in gates]
            layer = _upload(ctx, gates, log_in)
            try:
                out.fill(c, [None])
                ctx.fr_gkr_eval_layer_batch_dev(c, layer, inp.ptr(0), out.ptr(0), n)
                exp = ref.eval_layer_batch(gates, below, c.r)
                assert len(exp) == 1 << log_out and all(v == 0 for row in exp[n_gates:] for v in row)      # the zero rows
                assert np.array_equal(out.read(), out.expected(c, [_flat(exp)])), mode
                assert np.array_equal(inp.read(), inp.host), mode
            finally:
                ctx.gkr_layer_free(layer)
    finally:
        out.free()
        inp.free()


# ------------------------------------------------------------------------------------------- sum-check #1, call by call
def _check_sequence(ctx, c, gates, log_in, n, seed):
    """round 0, every bind-and-evaluate round and the closing call of one layer: evaluations, whole tables and finals"""
    r = c.r
    rows, n_gates = 1 << log_in, len(gates)
    log_out = (n_gates - 1).bit_length()
    ref_gates = [(g, o, a, b) for g, (o, a, b) in enumerate(gates)]
    vals, eq, w = _rows(c, rows, n, seed), _values(c, n, seed + 1), _values(c, 1 << log_out, seed + 2)
    assert all(v != 0 for v in w[n_gates:])                       # a nonzero tail: it must not be read
    layer = _upload(ctx, gates, log_in)
    bv, be, bw, bf = Bufs(ctx, 1, rows * n), Bufs(ctx, 1, n), Bufs(ctx, 1, 1 << log_out), Bufs(ctx, 1, rows)
    ints = lambda ev: tuple(codec.fr_from_mont(ev, c))            # noqa: E731
    try:
        bv.fill(c, [_flat(vals)])
        be.fill(c, [eq])
        bw.fill(c, [w])
        bf.fill(c, [None])
        args = (c, layer, bv.ptr(0), be.ptr(0), bw.ptr(0), n)
        length = n
        got = ctx.fr_gkr_dp_round_dev(*args, length)                                      # round 0: nothing changes
        assert ints(got) == ref.dp_round_evals(ref_gates, vals, eq, w, length, r), "round 0"
        assert np.array_equal(bv.read(), bv.host) and np.array_equal(be.read(), be.host)
        rnd = 0
        while length > 2:
            rnd += 1
            x = [0, r - 1][rnd - 1] if n == 8 and rnd <= 2 else rand_fr(r, 1, seed + 10 + rnd)[0]   # the challenge at its edges once
            got = ctx.fr_gkr_dp_round_dev(*args, length, bind=codec.fr_mont(x, c))
            vals, eq = [ref.dp_bind(t, length, x, r) for t in vals], ref.dp_bind(eq, length, x, r)
            length //= 2
            assert ints(got) == ref.dp_round_evals(ref_gates, vals, eq, w, length, r), rnd
            assert np.array_equal(bv.read(), bv.expected(c, [_flat(vals)])), rnd             # [length, 2 length) untouched
            assert np.array_equal(be.read(), be.expected(c, [eq])), rnd
        x = rand_fr(r, 1, seed + 9)[0]
        assert ctx.fr_gkr_dp_round_dev(*args, length, bind=codec.fr_mont(x, c), want_evals=False, finals_ptr=bf.ptr(0)) is None
        vals, eq = [ref.dp_bind(t, length, x, r) for t in vals], ref.dp_bind(eq, length, x, r)
        assert np.array_equal(bv.read(), bv.expected(c, [_flat(vals)]))
        assert np.array_equal(be.read(), be.expected(c, [eq]))
        assert np.array_equal(bf.read(), bf.expected(c, [[row[0] for row in vals]]))         # v_vec: every node, referenced or not
        assert np.array_equal(bw.read(), bw.host)
    finally:
        for b in (bv, be, bw, bf):
            b.free()
        ctx.gkr_layer_free(layer)


MIXED = [(0, 1, 2), (1, 0, 4), (1, 3, 3), (0, 4, 4), (1, 7, 0)]     # 5 gates (w has a tail), left == right, nodes 5 and 6 unread


# 2: round 0 and the closing call only; 8: both edge challenges; 64 / 128: half a wavefront / one; 512: one workgroup of columns;
# 1024: two, so the partial sums cross workgroups; every sequence ends below a wavefront
@pytest.mark.parametrize("n", [2, 4, 8, 64, 128, 512, 1024])
@pytest.mark.parametrize("curve", CURVES)
def test_rounds_over_the_copies(ctx, curve, n):
    assert n // 2 <= HYRAX_THREADS or n // 2 == 2 * HYRAX_THREADS
    _check_sequence(ctx, get_curve(curve), MIXED, 3, n, n)


@pytest.mark.parametrize("kind", ["one-gate", "all-add", "all-mul", "same-wire", "one-node-below"])
@pytest.mark.parametrize("curve", CURVES)
def test_rounds_gate_kinds(ctx, curve, kind):
    gates, log_in = {
        "one-gate": ([(1, 2, 1)], 2),
        "all-add": ([(0, a, b) for _, a, b in random_layers([16], 8, 1)[0]], 3),
        "all-mul": ([(1, a, b) for _, a, b in random_layers([16], 8, 2)[0]], 3),
        "same-wire": ([(o, a, a) for o, a, _ in random_layers([8], 8, 3)[0]], 3),
        "one-node-below": ([(1, 0, 0), (0, 0, 0), (1, 0, 0)], 0),     # the weight of gate 0 is 0
    }[kind]
    _check_sequence(ctx, get_curve(curve), gates, log_in, 16, len(kind))


# entries of the by-left-node list at each multiple of the chunk - 1, exact and + 1; 300 gates on one left node (above GKR_LONG, where
# the tables of gkr.hip change path) make one segment span several chunks
@pytest.mark.parametrize("n_gates", [HYRAX_CHUNK - 1, HYRAX_CHUNK, HYRAX_CHUNK + 1, 2 * HYRAX_CHUNK - 1, 2 * HYRAX_CHUNK, 2 * HYRAX_CHUNK + 1])
@pytest.mark.parametrize("curve", CURVES)
def test_rounds_chunk_boundaries(ctx, curve, n_gates):
    gates = random_layers([n_gates], 32, n_gates)[0]
    _check_sequence(ctx, get_curve(curve), gates, 5, 4, n_gates)


# HYRAX_THREADS chunks and one more over one workgroup of columns: gx = 1, gy = HYRAX_THREADS + 1 workgroups leave their partials, the
# fewest at which a thread of fr_sum_partials adds a second one; a chunk finds its node by binary search among about a thousand
# entries per node.  n = 2: round 0 (no bind) and the closing call; n = 4: also one bind-and-evaluate round over 257 workgroups
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("curve", CURVES)
def test_rounds_more_workgroups_than_sum_threads(ctx, curve, n):
    n_gates = HYRAX_THREADS * HYRAX_CHUNK + 1
    assert -(-n_gates // HYRAX_CHUNK) == HYRAX_THREADS + 1 and n // 2 <= HYRAX_THREADS
    gates = random_layers([n_gates], 8, n_gates)[0]
    _check_sequence(ctx, get_curve(curve), gates, 3, n, n_gates + n)


@pytest.mark.parametrize("curve", CURVES)
def test_rounds_hot_left_node(ctx, curve):
    assert 300 > GKR_LONG and 300 > 2 * HYRAX_CHUNK
    rng = np.random.default_rng(5)
    gates = [(int(rng.integers(0, 2)), 3, int(rng.integers(0, 16))) for _ in range(300)] + random_layers([40], 16, 6)[0]
    order = rng.permutation(len(gates))
    _check_sequence(ctx, get_curve(curve), [gates[i] for i in order], 4, 4, 300)


@pytest.mark.parametrize("curve", CURVES)
def test_round_errors_leave_everything_untouched(ctx, curve):
    c = get_curve(curve)
    log_in, n = 2, 8
    rows = 1 << log_in
    gates = [(0, 1, 2), (1, 0, 3), (1, 3, 3)]
    layer = _upload(ctx, gates, log_in)
    bufs = Bufs(ctx, 4, rows * n)                                  # v, eq, w, finals side by side (each longer than it needs)
    good = codec.fr_mont(5, c)
    big = np.frombuffer(c.r.to_bytes(32, "little"), dtype=np.uint64).copy()             # r: not reduced
    out = np.full((3, 4), SENT, dtype=np.uint64)
    kp = lambda a: None if a is None else V(a.ctypes.data)        # noqa: E731
    pv, pe, pw, pf = bufs.ptrs()
    try:
        bufs.fill(c, [_values(c, rows * n, i) for i in range(4)])

        def call(v=pv, eq=pe, w=pw, n=n, length=n, bind=good, ev=out, fin=None, layer=layer, cu=c.cid):
            return ctx.lib.zkp_fr_gkr_dp_round_dev(ctx.h, cu, V(layer), V(v), V(eq), V(w), n, length, kp(bind), kp(ev), V(fin))

        for kw in (dict(v=None), dict(eq=None), dict(w=None), dict(layer=None), dict(bind=None, ev=None),
                   dict(v=pv + 8), dict(eq=pe + 8), dict(w=pw + 8), dict(length=2, ev=None, fin=pf + 8),           # misaligned
                   dict(n=6), dict(n=0), dict(length=0), dict(length=6), dict(length=16), dict(n=1 << 27),           # sizes
                   dict(length=1), dict(length=1, ev=None), dict(length=2), dict(length=1, bind=None),                # too short
                   dict(bind=big),
                   dict(fin=pf), dict(length=4, ev=None, fin=pf), dict(length=2, bind=None, fin=pf),                   # finals: resulting length 1 only
                   dict(eq=pv), dict(eq=pv + 32 * (rows * n - 1)), dict(w=pv + 32), dict(w=pe + 32 * (n - 1)),         # overlaps
                   dict(length=2, ev=None, fin=pv + 32 * (rows * n - 1)), dict(length=2, ev=None, fin=pe), dict(length=2, ev=None, fin=pw)):
            assert call(**kw) == -1, kw
        assert call(cu=7) == -2
        assert np.array_equal(bufs.read(), bufs.host) and (out == SENT).all()
        # the batched layer evaluation: output over its input, misaligned, NULL, sizes
        ev = lambda i, p, k=n: ctx.lib.zkp_fr_gkr_eval_layer_batch_dev(ctx.h, c.cid, V(layer), V(i), V(p), k)    # noqa: E731
        assert ev(pv, pv) == -1 and ev(pv, pv + 32 * (rows * n - 1)) == -1 and ev(pv, pe + 8) == -1 and ev(pv + 8, pe) == -1
        assert ev(None, pe) == -1 and ev(pv, None) == -1 and ev(pv, pe, 0) == -1 and ev(pv, pe, 6) == -1 and ev(pv, pe, 1 << 27) == -1
        assert ctx.lib.zkp_fr_gkr_eval_layer_batch_dev(ctx.h, 7, V(layer), V(pv), V(pe), n) == -2
        assert np.array_equal(bufs.read(), bufs.host)
        assert call(bind=None) == 0 and call() == 0 and call(length=4) == 0 and call(length=2, ev=None, fin=pf) == 0
    finally:
        bufs.free()
        ctx.gkr_layer_free(layer)


# ------------------------------------------------------------------------------------------- the driver
def _golden(name):
    def make(r, n):
        case = load_golden()[name]
        inputs, witnesses = assignments(case, n, r, 31)
        return case["num_inputs"], case["num_aux"], case["layers"], [[v % r for v in row] for row in inputs], [[v % r for v in row] for row in witnesses]
    return make


def _random3(r, n):
    layers = random_layers([16, 8, 2], 16, 9)                      # three layers over 8 witnesses and 8 inputs
    return 8, 8, layers, [rand_fr(r, 8, 50 + t) for t in range(n)], [rand_fr(r, 8, 150 + t) for t in range(n)]


CASES = {"mini": _golden("mini"), "test": _golden("test"), "random-3": _random3}


@pytest.mark.parametrize("n", [4, 64])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("curve", CURVES)
def test_driver_equals_the_literal_reference(ctx, curve, case, n):
    c = get_curve(curve)
    r = c.r
    num_inputs, num_aux, layers_raw, inputs, witnesses = CASES[case](r, n)
    rc = gkr_ref.Circuit(num_inputs, num_aux, layers_raw)
    q, qa = points(r, rc.layers[-1].bit_size, n.bit_length() - 1, 7)
    exp_proofs, exp_evals, exp_u, exp_points = ref.prover(rc, inputs, witnesses, qa, q, *callbacks(r), r, sumcheck=ref.sumcheck_literal)
    circuit = gkr.Circuit(ctx, num_inputs, num_aux, layers_raw)
    evals = None
    try:
        evals = hyrax.evaluate_batch(circuit, c, inputs, witnesses)
        assert [hyrax.read_layer(circuit, c, evals, d, n) for d in range(circuit.depth)] == exp_evals
        result_u = hyrax.eval_outputs(circuit, c, evals, n, q, qa)
        assert result_u == exp_u
        proofs, q_aside, ql, qr = hyrax.prove_layers(circuit, c, evals, n, qa, q, result_u, *callbacks(r))
        assert proofs == exp_proofs and (q_aside, ql, qr) == exp_points           # every coefficient, challenge and (x, y)
        assert [hyrax.read_layer(circuit, c, evals, d, n) for d in range(circuit.depth)] == exp_evals      # the layers are inputs
        assert ref.verify(rc, proofs, exp_evals[-1], exp_evals[0], qa, q, *callbacks(r), r)
        assert hyrax.eval_witness(ctx, c, witnesses, q_aside, ql, qr) == ref.eval_witness(witnesses, q_aside, ql, qr, r)
    finally:
        if evals is not None:
            gkr.free_evals(circuit, evals)
        circuit.free()


def test_driver_one_copy_and_rules(ctx):
    c = get_curve("bn254")
    r = c.r
    layers_raw = random_layers([8, 4, 1], 8, 12)
    inputs, witnesses = [rand_fr(r, 4, 1)], [rand_fr(r, 4, 2)]
    rc = gkr_ref.Circuit(4, 4, layers_raw)
    q, qa = points(r, 0, 0, 7)
    exp_proofs, exp_evals, exp_u, exp_points = ref.prover(rc, inputs, witnesses, qa, q, *callbacks(r), r)
    circuit = gkr.Circuit(ctx, 4, 4, layers_raw)
    evals = hyrax.evaluate_batch(circuit, c, inputs, witnesses)
    try:
        assert hyrax.eval_outputs(circuit, c, evals, 1, q, qa) == exp_u
        proofs, *pts = hyrax.prove_layers(circuit, c, evals, 1, qa, q, exp_u, *callbacks(r))      # n = 1: no sum-check #1
        assert proofs == exp_proofs and tuple(pts) == exp_points
        with pytest.raises(ValueError, match="power of two"):
            hyrax.evaluate_batch(circuit, c, inputs * 3, witnesses * 3)
    finally:
        gkr.free_evals(circuit, evals)
        circuit.free()
    circuit = gkr.Circuit(ctx, 2, 2, [[(0, 0, 1), (1, 1, 2), (1, 3, 3)], [(0, 0, 2)]])          # a layer of three gates
    evals = hyrax.evaluate_batch(circuit, c, [[1, 2], [3, 4]], [[5, 6], [7, 8]])
    try:
        with pytest.raises(ValueError, match="power-of-two"):
            hyrax.prove_layers(circuit, c, evals, 2, [1], [], 0, *callbacks(r))
    finally:
        gkr.free_evals(circuit, evals)
        circuit.free()
