"""CPU: tests/plonk_open_ref.py against the identities it must satisfy: the verifier's equality check on the eleven evaluations,
the opening relations of both witness polynomials at a random point, and the golden file of the mini circuit."""
import json

import pytest

from tests import plonk_open_ref as oref
from tests import plonk_ref as ref
from tests.plonk_cases import KS, MINI_CHALLENGES, challenges, mini_circuit, rand_fr, random_circuit

CASES = [("bls12_381", "mini", 8)] + [(curve, gates, n) for curve in ("bn254", "bls12_381") for gates, n in ((37, 64), (300, 512))]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def case(request):
    """(index, public inputs, challenges, zeta, weights, everything after round 3); computed once per case, never modified"""
    curve, kind, n = request.param
    cs = ref.RefComposer(curve)
    if kind == "mini":
        mini_circuit(cs)
        ch = (MINI_CHALLENGES["beta"], MINI_CHALLENGES["gamma"], MINI_CHALLENGES["alpha"])
    else:
        random_circuit(cs, kind, 60 + kind)
        ch = challenges(cs.r, kind)
    ix = ref.RefIndex(cs, KS)
    assert ix.n == n
    polys = ref.prove_rounds(ix, cs.synthesize(), cs.public_inputs(), *ch)
    assert polys["closes"]
    zeta, tau = rand_fr(cs.r, 2, 900 + n)
    weights = dict(zip(oref.AT_ZETA, rand_fr(cs.r, len(oref.AT_ZETA), 901 + n)))
    return ix, cs.public_inputs(), ch, zeta, tau, weights, oref.run(ix, polys, cs.public_inputs(), *ch, zeta, weights)


def test_labels_are_the_reference_order():
    assert list(oref.LABELS) == sorted(oref.LABELS) and len(oref.LABELS) == 11
    assert len(oref.BASE) == 20 and len(set(oref.BASE)) == 20 and len(oref.AT_ZETA) == 10


def test_equality_check_holds(case):
    ix, pi, ch, zeta, _, _, out = case
    assert list(out["evals"]) == list(oref.LABELS)
    assert len(out["terms"]) == 8 and [label for _, label in out["terms"]] == ["q_0", "q_1", "q_2", "q_3", "q_m", "q_c", "z", "sigma_3"]
    assert oref.equality_check(ix, out["evals"], pi, *ch, zeta)
    # pi(zeta) in Lagrange form is the interpolated polynomial at zeta
    padded = list(pi) + [0] * (ix.n - len(pi))
    assert oref.pi_at(ix, pi, zeta) == ref.horner(ix.dn.ifft(padded), zeta, ix.r)
    # r(zeta) by linearity is the linearisation polynomial at zeta
    assert ref.horner(out["r_poly"], zeta, ix.r) == out["evals"]["r"]


@pytest.mark.parametrize("label", oref.LABELS)
def test_equality_check_fails_on_a_changed_evaluation(case, label):
    ix, pi, ch, zeta, _, _, out = case
    bad = dict(out["evals"])
    bad[label] = (bad[label] + 1) % ix.r
    # q_arith(zeta) enters the check only as q_arith(zeta) pi(zeta) (verifier.rs:140): without a public input (the mini circuit)
    # the check cannot see it, in the reference as here; every other evaluation is always seen
    blind = label == "q_arith" and not any(v % ix.r for v in pi)
    assert oref.equality_check(ix, bad, pi, *ch, zeta) == blind
    if label == "q_arith":
        assert blind == (ix.n == 8)


def test_openings(case):
    ix, _, _, zeta, tau, _, out = case
    r, n = ix.r, ix.n
    assert len(out["w_zeta"]) == n - 1 and len(out["w_shifted"]) == n - 1
    v = out["combined_value"]
    assert out["w_zeta_rem"] == v
    assert (ref.horner(out["combined"], tau, r) - v) % r == ref.horner(out["w_zeta"], tau, r) * (tau - zeta) % r
    vs, zs = out["evals"]["z"], zeta * ix.dn.group_gen % r
    assert out["w_shifted_rem"] == vs
    assert (ref.horner(out["table"]["z"], tau, r) - vs) % r == ref.horner(out["w_shifted"], tau, r) * (tau - zs) % r


def test_golden_regenerates():
    assert json.dumps(oref.make_golden(), indent=1) + "\n" == oref.GOLDEN.read_text()
    g = oref.load_golden()
    assert list(g["evaluations"]) == list(oref.LABELS) and len(g["r_terms"]) == 8
    assert len(g["w_zeta"]) == g["n"] - 1 == len(g["w_shifted_zeta"])
