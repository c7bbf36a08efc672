"""CPU: tests/hyrax_ref.py against itself.  The literal restatement of ZkSumcheckProof::prover's table work (the G x n temp_vec, the
per-gate left_eq / right_eq vectors) equals the reduced form (one eq table, one weight vector, Libra's bookkeeping tables) on every
coefficient, challenge and (x, y); the plain verifier accepts both and rejects a proof with one value changed; the circuits of
hyrax/tests/mini.rs and hyrax/tests/test.rs keep their recorded round polynomials."""
import pytest

from ckb_zkp_amd.params import get_curve
from tests import gkr_ref, hyrax_ref as ref
from tests.gkr_cases import rand_fr, random_layers
from tests.hyrax_cases import callbacks, load_golden, points

R = get_curve("bn254").r

# (log n, log ng, log G) of one layer
SHAPES = [(0, 1, 0), (1, 1, 1), (2, 3, 2), (3, 2, 3), (3, 3, 0), (1, 3, 3), (0, 0, 0), (2, 0, 1)]


def _layer(log_n, log_ng, log_g, seed):
    n, ng, g = 1 << log_n, 1 << log_ng, 1 << log_g
    gates = [(i, op, a, b) for i, (op, a, b) in enumerate(random_layers([g], ng, seed)[0])]
    rows = [rand_fr(R, n, seed + 10 + i) for i in range(ng)]
    q_vec = (rand_fr(R, log_n, seed + 1), rand_fr(R, log_g, seed + 2), rand_fr(R, log_g, seed + 3))
    u = tuple(rand_fr(R, 2, seed + 4))
    return n, ng, gates, rows, q_vec, u


def _claim(u, q_vec, gates, rows, n):
    """what the layer's sum-check proves: sum_t eq(q')[t] sum_g w[g] op_g(V[left][t], V[right][t])"""
    eq, w = ref.eval_eq(q_vec[0], R), ref.weights(u, q_vec[1], q_vec[2], R)
    return sum(eq[t] * w[g] * ref._op(op, rows[a][t], rows[b][t]) for g, op, a, b in gates for t in range(n)) % R


@pytest.mark.parametrize("shape", SHAPES)
def test_literal_equals_fast_on_one_layer(shape):
    n, ng, gates, rows, q_vec, u = _layer(*shape, seed=sum(shape) * 7 + shape[0])
    claim = _claim(u, q_vec, gates, rows, n)
    lit = ref.sumcheck_literal(claim, u, q_vec, gates, rows, n, ng, callbacks(R)[0], R)
    fast = ref.sumcheck_fast(claim, u, q_vec, gates, rows, n, ng, callbacks(R)[0], R)
    assert lit == fast
    polys, rs, r0, r1, _ = lit
    assert [len(p) for p in polys] == [4] * shape[0] + [3] * (2 * shape[1])
    assert (len(rs), len(r0), len(r1)) == (shape[0], shape[1], shape[1])
    for p in polys[:1]:                                            # the first round really sums to the claim
        assert (ref.poly_evaluate(p, 0, R) + ref.poly_evaluate(p, 1, R)) % R == claim


def test_literal_rejects_a_gate_count_that_is_no_power_of_two():
    n, ng, gates, rows, q_vec, u = _layer(1, 2, 2, seed=3)
    with pytest.raises(AssertionError):
        ref.sumcheck_literal(0, u, q_vec, gates[:3], rows, n, ng, callbacks(R)[0], R)


def _random_case(widths, below, n, seed):
    layers = random_layers(widths, 2 * below, seed)
    inputs = [rand_fr(R, below - 1, seed + 2 * t + 1) for t in range(n)]
    witnesses = [rand_fr(R, below, seed + 2 * t + 2) for t in range(n)]
    return gkr_ref.Circuit(below - 1, below, layers), inputs, witnesses


@pytest.mark.parametrize("widths,below,n", [([4, 2, 1], 2, 1), ([8, 4, 2], 4, 4), ([2, 8, 4, 1], 2, 8)])
def test_whole_prover_literal_equals_fast_and_verifies(widths, below, n):
    circuit, inputs, witnesses = _random_case(widths, below, n, seed=len(widths) + n)
    q, qa = points(R, circuit.layers[-1].bit_size, n.bit_length() - 1, 5)
    lit = ref.prover(circuit, inputs, witnesses, qa, q, *callbacks(R), R, sumcheck=ref.sumcheck_literal)
    fast = ref.prover(circuit, inputs, witnesses, qa, q, *callbacks(R), R, sumcheck=ref.sumcheck_fast)
    assert lit == fast
    proofs, evals, result_u, (q_aside, ql, qr) = lit
    assert [[row[t] for row in evals[-1][:widths[-1]]] for t in range(n)] == \
        [gkr_ref.circuit_evaluate(circuit, i, w, R)[-1] for i, w in zip(inputs, witnesses)]
    assert ref.verify(circuit, proofs, evals[-1], evals[0], qa, q, *callbacks(R), R)
    assert proofs[-1][1] == (q_aside, ql, qr)
    # the witness openings of hyrax_proof.rs:149-178 agree with (x, y) as the verifier combines them (:304-313)
    ew = ref.eval_witness(witnesses, q_aside, ql, qr, R)
    half = len(evals[0]) // 2
    inp_vec = [v for t in range(n) for v in [evals[0][half + i][t] for i in range(half)]]
    for point, wit, got in ((ql, ew[0], proofs[-1][2][0]), (qr, ew[1], proofs[-1][2][1])):
        ei = gkr_ref.eval_value(inp_vec, list(q_aside) + list(point[1:]), R)
        assert got == ((1 - point[0]) * wit + point[0] * ei) % R


def test_verifier_rejects_one_changed_value():
    circuit, inputs, witnesses = _random_case([8, 4, 2], 4, 4, seed=11)
    q, qa = points(R, 1, 2, 6)
    proofs, evals, _, _ = ref.prover(circuit, inputs, witnesses, qa, q, *callbacks(R), R, sumcheck=ref.sumcheck_fast)
    check = lambda p: ref.verify(circuit, p, evals[-1], evals[0], qa, q, *callbacks(R), R)    # noqa: E731
    assert check(proofs)
    for layer in range(len(proofs)):
        polys, chal, (x, y) = proofs[layer]
        swap = lambda new: proofs[:layer] + [new] + proofs[layer + 1:]                      # noqa: E731
        for k in range(len(polys)):                                # one coefficient of every round polynomial
            for j in range(len(polys[k])):
                bad = [list(p) for p in polys]
                bad[k][j] = (bad[k][j] + 1) % R
                assert not check(swap((bad, chal, (x, y)))), (layer, k, j)
        assert not check(swap((polys, chal, ((x + 1) % R, y)))), layer
        assert not check(swap((polys, chal, (x, (y + 1) % R)))), layer
    assert not check(proofs[:-1])
    other = [[(v + 1) % R for v in row] for row in evals[-1]]
    assert not ref.verify(circuit, proofs, other, evals[0], qa, q, *callbacks(R), R)


@pytest.mark.parametrize("name", ["mini", "test"])
def test_golden_circuits(name):
    case = load_golden()[name]
    r = get_curve(case["curve"]).r
    circuit = gkr_ref.Circuit(case["num_inputs"], case["num_aux"], case["layers"])
    n = len(case["inputs"])
    assert n == {"mini": 2, "test": 4}[name]
    q, qa = points(r, circuit.layers[-1].bit_size, n.bit_length() - 1, 7)
    lit = ref.prover(circuit, case["inputs"], case["witnesses"], qa, q, *callbacks(r), r, sumcheck=ref.sumcheck_literal)
    assert lit == ref.prover(circuit, case["inputs"], case["witnesses"], qa, q, *callbacks(r), r, sumcheck=ref.sumcheck_fast)
    proofs, evals, _, _ = lit
    if name == "mini":                                             # (3 + 0) (2 * 2) + (0 * 2) (2 * 2) in copy 0
        assert evals[-1][0][0] == 12
    assert [polys for polys, _, _ in proofs] == case["pins"]
    assert ref.verify(circuit, proofs, evals[-1], evals[0], qa, q, *callbacks(r), r)
