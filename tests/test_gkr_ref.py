"""CPU: tests/gkr_ref.py (the Python-integer restatement of Libra's linear GKR that the device tests compare against) proves and
verifies the instance of libra/tests/mini.rs and random layered circuits, and its tables satisfy the identities that tie them to
Layer::eval_operators and eval_value."""
import pytest

from ckb_zkp_amd.params import get_curve
from tests import gkr_ref as ref
from tests.gkr_cases import callbacks, load_mini, rand_fr, random_layers


def _prove_and_check(layers_raw, inputs, aux, r, seed):
    circuit = ref.Circuit(len(inputs), len(aux), layers_raw)
    gu0 = gu = rand_fr(r, circuit.layers[-1].bit_size, seed)
    log = []

    def recording(cb):
        nr, af, ab = cb

        def next_round(coeffs):
            x = nr(coeffs)
            log.append(("round", x))
            return x

        def next_alpha_beta():
            v = ab()
            log.append(("ab", v))
            return v

        return next_round, af, next_alpha_beta

    proofs, output, evals, ru, rv = ref.prover(circuit, inputs, aux, gu, *recording(callbacks(r)), r)
    assert len(proofs) == circuit.depth - 1
    assert ref.verify(circuit, proofs, output, evals[0], gu, *callbacks(r), r)
    # the final values against their definitions, layer by layer, with the challenges the prover drew
    alpha, beta, gv = 1, 0, [0] * len(gu)
    it = iter(log)
    for i, (polys_1, finals_1, polys_2, finals_2) in enumerate(proofs):
        d = circuit.depth - 1 - i
        k = circuit.layers[d - 1].bit_size
        assert len(polys_1) == len(polys_2) == k and all(len(p) == 3 for p in polys_1 + polys_2)
        lru = [next(it)[1] for _ in range(k)]
        lrv = [next(it)[1] for _ in range(k)]
        add_ev, mul_ev = ref.eval_operators(circuit.layers[d], gu, gv, lru, lrv, alpha, beta, r)     # circuit.rs:82-108
        assert (finals_2[1], finals_2[2]) == (mul_ev, add_ev)
        assert finals_1[0] == ref.eval_value(evals[d - 1], lru, r) and finals_2[0] == ref.eval_value(evals[d - 1], lrv, r)
        if d > 1:
            gu, gv = lru, lrv
            alpha, beta = (v % r for v in next(it)[1])
    assert (lru, lrv) == (ru, rv)
    return circuit, proofs, output, evals, gu0


def test_mini_instance_proves_and_verifies():
    curve, layers_raw, inputs, witnesses = load_mini()
    assert curve == "bls12_381"
    r = get_curve(curve).r
    circuit, proofs, output, evals, _ = _prove_and_check(layers_raw, inputs, witnesses, r, 1)
    assert [l.bit_size for l in circuit.layers] == [3, 2, 1, 0]
    assert evals[0] == [2, 3, 0, 0, 2, r - 10, 1, 0]                  # aux, then inputs (circuit.rs:153-156)
    assert evals[1:] == [[3, 4, 0, 4], [12, 0], [12]] and output == [12]   # by hand from the gate list


# gates per layer, input layer below: every layer a power of two except the output; a one-gate output; a one-gate middle layer
@pytest.mark.parametrize("widths,hot", [([8, 4, 2, 1], None), ([64, 32, 32, 3], None), ([2, 2, 2], None), ([16, 1], None),
                                        ([4, 1, 2], None), ([128, 64, 16, 16, 5], (2, 7, 0.5))])
@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_random_circuits_prove_and_verify(curve, widths, hot):
    r = get_curve(curve).r
    seed = sum(widths)
    inputs, aux = rand_fr(r, 5, seed), rand_fr(r, 7, seed + 1)
    inputs[0], aux[0] = r - 1, 0
    _prove_and_check(random_layers(widths, 16, seed, hot), inputs, aux, r, seed + 2)


def test_tampered_polynomial_is_rejected():
    r = get_curve("bn254").r
    layers_raw = random_layers([8, 4, 3], 8, 5)
    inputs, aux = rand_fr(r, 4, 6), rand_fr(r, 4, 7)
    circuit, proofs, output, evals, gu = _prove_and_check(layers_raw, inputs, aux, r, 8)
    for layer, phase, coeff in ((0, 0, 0), (1, 2, 1), (1, 0, 2)):
        bad = [tuple([list(p) for p in part] if i in (0, 2) else list(part) for i, part in enumerate(pr)) for pr in proofs]
        bad[layer][phase][0][coeff] = (bad[layer][phase][0][coeff] + 1) % r
        assert not ref.verify(circuit, bad, output, evals[0], gu, *callbacks(r), r)
    bad = [tuple([list(p) for p in part] if i in (0, 2) else list(part) for i, part in enumerate(pr)) for pr in proofs]
    bad[-1][1][0] = (bad[-1][1][0] + 1) % r                                                          # f(ru) of the input layer
    assert not ref.verify(circuit, bad, output, evals[0], gu, *callbacks(r), r)
    assert not ref.verify(circuit, proofs, [(output[0] + 1) % r] + output[1:], evals[0], gu, *callbacks(r), r)


def test_layer_rules():
    with pytest.raises(ValueError, match="IllegalOperator"):
        ref.Circuit(2, 2, [[(2, 0, 1)]])
    with pytest.raises(ValueError, match="IllegalNode"):
        ref.Circuit(2, 2, [[(0, 0, 4)]])
    assert ref.eval_layer([(0, 0, 1), (1, 1, 1), (1, 0, 1)], [3, 5], 7) == [1, 4, 1, 0]


@pytest.mark.parametrize("period", [7, 16])
def test_periodic_round_helpers_equal_the_direct_sums(period):
    """tests/util.periodic_round_sums / periodic_bind, on which the device tests of long tables rest, against the round functions of
    gkr_ref and sumcheck_ref over the spelled-out tables (h = 32: four whole periods and four residues more, or two whole periods)"""
    from tests import sumcheck_ref
    from tests.util import periodic_bind, periodic_round_sums
    r = get_curve("bn254").r
    n = 64
    bases = [rand_fr(r, period, 70 + s) for s in range(4)]
    tables = [[b[j % period] for j in range(n)] for b in bases]
    for phase, fu in ((1, None), (2, 12345)):
        nt = 5 - phase
        got = periodic_round_sums(lambda t: ref.round_evals(phase, t, fu, r), bases[:nt], n // 2, r)     # noqa: B023
        assert got == ref.round_evals(phase, tables[:nt], fu, r)
    for kind, arity in sumcheck_ref.ARITY.items():
        got = periodic_round_sums(lambda t: sumcheck_ref.round_evals(kind, t, r), bases[:arity], n // 2, r)   # noqa: B023
        assert got == sumcheck_ref.round_evals(kind, tables[:arity], r)
    for b, t in zip(bases, tables):
        block = periodic_bind(b, n // 2, 99, r)
        assert [block[j % period] for j in range(n // 2)] == sumcheck_ref.combine_with_r(t, 99, r)
