"""CPU: the Python reference of the Bulletproofs R1CS prover and verifier (tests/bulletproofs_ref.py) is consistent with itself and
with the golden proof of the reference's `mini` circuit.  The reference verifier accepts what the reference prover makes and rejects
it after a change of t_x, of one element of l_x, of one L point or of the public input; t(x) = <l(x), r(x)>.  The golden file pins
this Python reference (a regression pin, not parity with the Rust crate)."""
import copy

import numpy as np
import pytest

from ckb_zkp_amd import codec
from ckb_zkp_amd.params import get_curve
from tests import bulletproofs_ref as ref
from tests.bulletproofs_cases import (MINI_CURVE, Challenger, assert_same_proof, load_golden, mini, mini_setup, proof_to_json,
                                      random_circuit, randomness)

CURVES = ["bn254", "bls12_381"]
_PROOFS = {}


def _mini_proof(curve):
    """one proof per curve, shared and never changed (the tests copy it)"""
    if curve not in _PROOFS:
        cs, ints, _, rand = mini_setup(curve)
        _PROOFS[curve] = (cs, ints, ref.prove(curve, cs, ints, rand, Challenger(curve)))
    return _PROOFS[curve]


@pytest.mark.parametrize("curve", CURVES)
def test_mini_is_accepted_and_tampering_is_rejected(curve):
    c = get_curve(curve)
    cs, ints, proof = _mini_proof(curve)
    assert (cs.num_constraints(), cs.num_aux, len(proof.l_x), len(proof.L_vec)) == (10, 2, 16, 4)
    assert ref.verify(curve, cs, ints, proof, [10], Challenger(curve))
    bad = copy.deepcopy(proof)
    bad.t_x = (bad.t_x + 1) % c.r
    assert not ref.verify(curve, cs, ints, bad, [10], Challenger(curve))
    bad = copy.deepcopy(proof)
    bad.l_x[5] = codec.fr_mont((codec.fr_int(bad.l_x[5], c) + 1) % c.r, c)
    assert not ref.verify(curve, cs, ints, bad, [10], Challenger(curve))
    bad = copy.deepcopy(proof)
    bad.L_vec[1] = bad.R_vec[1]
    assert not ref.verify(curve, cs, ints, bad, [10], Challenger(curve))
    assert not ref.verify(curve, cs, ints, proof, [11], Challenger(curve))
    assert ref.verify(curve, cs, ints, proof, [10], Challenger(curve))      # the shared proof is unchanged


@pytest.mark.parametrize("curve", CURVES)
def test_t_of_x_is_the_inner_product(curve):
    c = get_curve(curve)
    r = c.r
    for cs in (mini(curve), random_circuit(curve, 2, 5, 7)):
        rand = randomness(curve, cs, 3)
        n_max = max(cs.num_constraints(), cs.num_aux)
        y, z, x = 0x1234567, r - 2, r - 5
        lp, rp = ref.lr_polys(cs, rand[:n_max], rand[n_max:2 * n_max], y, z)
        t = ref.t_coeffs(lp, rp, r)
        assert sorted(t) == list(range(2, 11))
        l_x, r_x = ref.eval_vec_poly(lp, x, r), ref.eval_vec_poly(rp, x, r)
        assert sum(t[d] * pow(x, d, r) for d in t) % r == ref.dot(l_x, r_x, r)
        # a satisfied system: t_4 is what the verifier computes on its own, delta + <z_Q, c>
        Y, Z, zn, U = ref._yz_vectors(y, z, cs.num_constraints(), len(l_x), r)
        s = cs.input_assignment
        zq_c = sum(Z[i] * sum(v * s[col] for col, v in row.items() if col < cs.num_inputs)
                   for i, row in enumerate(ref._combined(cs, zn, r))) % r
        assert t[4] == (ref.dot(U, Z, r) + zq_c) % r


def test_mini_proof_equals_the_golden_file():
    _, _, proof = _mini_proof(MINI_CURVE)
    assert proof_to_json(proof, MINI_CURVE) == load_golden()


def test_a_second_run_gives_the_same_proof():
    cs, ints, _, rand = mini_setup("bn254")
    again = ref.prove("bn254", cs, ints, rand, Challenger("bn254"))
    assert_same_proof(again, _mini_proof("bn254")[2])
    assert np.array_equal(again.l_x, _mini_proof("bn254")[2].l_x)
