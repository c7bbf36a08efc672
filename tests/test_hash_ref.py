"""CPU: the Python-integer restatement of the hashes and of CBMT (tests/hash_ref.py) against its own algebra, against a second
route to each result, and against the witness of the headline circuit.  The GPU tests compare the device with this module."""
import random

import pytest

from ckb_zkp_amd import hashes, merkle
from ckb_zkp_amd.circuits import MIMC_ROUNDS, mimc_chain_instance
from ckb_zkp_amd.params import get_curve
from tests import hash_cases as cases
from tests import hash_ref as ref

CURVES = ["bn254", "bls12_381"]


@pytest.mark.parametrize("alpha", [3, 5, 7])
@pytest.mark.parametrize("curve", CURVES)
def test_the_inverse_sbox_undoes_the_sbox(curve, alpha):
    r = get_curve(curve).r
    if (r - 1) % alpha == 0:
        with pytest.raises(ValueError):
            hashes.rescue_inv_alpha(curve, alpha)
        return
    inv = hashes.rescue_inv_alpha(curve, alpha)
    assert 0 < inv < r - 1 and alpha * inv % (r - 1) == 1
    rng = random.Random(alpha)
    for x in [0, 1, 2, r - 1] + [rng.randrange(r) for _ in range(8)]:
        assert pow(pow(x, alpha, r), inv, r) == x and pow(pow(x, inv, r), alpha, r) == x


def test_alpha_5_has_an_inverse_on_both_curves_and_bn254_gives_the_reference_exponent():
    for curve in CURVES:
        assert (get_curve(curve).r - 1) % 5 != 0
    # rescue.rs:25-30 writes this exponent as four words; it is 5^-1 mod (r - 1), nothing more
    assert hashes.rescue_inv_alpha("bn254", 5) == 0x26b6a528b427b35493736af8679aad17535cb9d394945a0dcfe7f7a98ccccccd


@pytest.mark.parametrize("curve", CURVES)
def test_poseidon_with_every_round_full_is_the_unflagged_permutation(curve):
    p = cases.poseidon_params(curve, [1] * 12)
    rng = random.Random(12)
    for _ in range(4):
        xl, xr = rng.randrange(p["r"]), rng.randrange(p["r"])
        assert ref.block(p, xl, xr) == ref.poseidon_block_all_full(xl, xr, p["ark"], p["mds"], p["alpha"], p["r"])
    # and a partial round is not a full one
    q = dict(p, full=[1] * 6 + [0] + [1] * 5)
    assert ref.block(q, 1, 2) != ref.block(p, 1, 2)


def test_schedules():
    ref_s = hashes.poseidon_reference_schedule(cases.REF_POSEIDON_ROUNDS, cases.REF_POSEIDON_RF)
    assert len(ref_s) == 91 and ref_s.count(0) == 1 and ref_s[4] == 0                 # poseidon.rs:560
    std = hashes.poseidon_schedule(4, cases.REF_POSEIDON_RP, 4)
    assert len(std) == 91 and std[:4] == [1] * 4 and std[-4:] == [1] * 4 and std.count(0) == 83


@pytest.mark.parametrize("kind", ["mimc", "poseidon"])
def test_queue_root_equals_the_tree_root(kind):
    p = cases.mimc_params("bn254", 3) if kind == "mimc" else cases.poseidon_params("bn254", [1, 0, 1])
    rng = random.Random(33)
    for merge in (ref.merge_block(p), ref.merge_chain(p)):
        for n in range(1, 34):
            leaves = [rng.randrange(p["r"]) for _ in range(n)]
            nodes = ref.build_tree(leaves, merge)
            assert len(nodes) == 2 * n - 1 and nodes[n - 1:] == leaves
            assert ref.build_merkle_root(leaves, merge) == nodes[0], n
    assert ref.build_tree([], merge) == [] and ref.build_merkle_root([], merge) == 0


def test_tree_and_proof_on_the_recorded_integers_of_the_reference_tests():
    """cbmt.rs:253-338 with merge = right - left: the node vectors and the lemmas its tests assert"""
    sub = lambda left, right: right - left                      # noqa: E731
    assert ref.build_tree([1], sub) == [1]
    assert ref.build_tree([1, 2], sub) == [1, 1, 2]
    assert ref.build_tree([2, 3, 5, 7, 11], sub) == [4, -2, 2, 4, 2, 3, 5, 7, 11]
    assert ref.build_merkle_root([2, 3, 5, 7, 11], sub) == 4
    nodes = ref.build_tree([2, 3, 5, 7, 11, 13], sub)
    index, lemmas = ref.build_proof(nodes, 5)
    assert lemmas == [11, 2, 1] and ref.proof_root(index, lemmas, 13, sub) == 1
    assert ref.build_proof([2], 0) == (0, []) and ref.proof_root(0, [], 2, sub) == 2
    assert ref.build_proof(nodes, 6) is None and ref.build_proof([], 0) is None


@pytest.mark.parametrize("n", [1, 2, 3, 5, 10])
def test_proof_root_recovers_the_root_for_every_leaf(n):
    p = cases.mimc_params("bls12_381", 4)
    rng = random.Random(n)
    leaves = [rng.randrange(p["r"]) for _ in range(n)]
    for merge in (ref.merge_block(p), ref.merge_chain(p)):
        nodes = ref.build_tree(leaves, merge)
        for leaf in range(n):
            index, lemmas = ref.build_proof(nodes, leaf)
            assert index == n - 1 + leaf and len(lemmas) == merkle.depth(index)
            assert ref.proof_root(index, lemmas, leaves[leaf], merge) == nodes[0]
            if lemmas:
                assert ref.proof_root(index, lemmas, (leaves[leaf] + 1) % p["r"], merge) != nodes[0]
        assert ref.build_proof(nodes, n) is None


@pytest.mark.parametrize("curve", CURVES)
def test_mimc_trace_is_the_witness_of_the_headline_circuit(curve):
    inst = mimc_chain_instance(curve, 7)
    r = get_curve(curve).r
    assert len(inst.constants) == MIMC_ROUNDS
    want = []
    for xl, xr in inst.preimages:
        row = ref.mimc_trace(xl, xr, inst.constants, r)
        assert len(row) == 2 * MIMC_ROUNDS + 2 and row[-1] == ref.mimc_block(xl, xr, inst.constants, r)
        want += row
    assert inst.z[0] == 1 and inst.z[1:] == want


def test_hash_elements_returns_the_gadgets_triple():
    p = cases.mimc_params("bn254", 5)
    msg = [3, 1, 4, 1, 5]
    xl, xr, image = ref.hash_elements(p, msg)
    assert xr == 5 and image == ref.block(p, xl, xr) and xl == ref.hash_elements(p, msg[:4])[2]
    assert ref.hash_elements(p, [9]) == (0, 9, ref.block(p, 0, 9))


def test_products_of_a_block_match_the_counts_the_design_quotes():
    assert ref.products_of_block(cases.mimc_params("bn254", 322)) == 644
    ref_s = hashes.poseidon_reference_schedule(91, 8)
    assert ref.products_of_block(cases.poseidon_params("bn254", ref_s)) == 90 * 18 + 12
    assert 22000 < ref.products_of_block(cases.rescue_params("bn254", 22)) < 26000
