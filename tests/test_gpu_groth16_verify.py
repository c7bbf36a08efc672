"""groth16.prepare_verifying_key / verify_proof / verify_proofs_batch on the device: the reference's own acceptance predicate
(`verify_proof(..) == true`, groth16/tests/mini.rs:89,96) on device proofs, agreement with the oracle's verifier on the same proof,
rejection of a wrong public input, of 2A in place of A and of -C, MalformedVerifyingKey on a wrong input count; the batch check over
1, 2 and 65 proofs with distinct r, s and inputs, with all coefficients 1 and with seeded random ones, and one tampered proof of 65
located by verify_proof."""
import random
from types import SimpleNamespace

import pytest

from ckb_zkp_amd import codec, groth16
from ckb_zkp_amd.circuits import Mini, mimc_chain_instance, samples_for_domain
from ckb_zkp_amd.r1cs import SynthesisError
from oracle.pyref import pairing as opairing
from oracle.pyref.curves import Group
from tests.util import OC

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
TOXIC = dict(alpha=0x1234567890ABCDEF1, beta=0xFEDCBA09876543211, gamma=0x1111111111111111111,
             delta=0x2222222222222222223, tau=0x3333333333333333335)


def oracle_vk(params):
    """the verifying key as the oracle's verify_proof reads it: canonical integers"""
    c = params.curve
    one1 = lambda a: codec.g1_from_mont(a.reshape(1, -1), None, c)[0]
    one2 = lambda a: codec.g2_from_mont(a.reshape(1, -1), None, c)[0]
    return SimpleNamespace(alpha_g1=one1(params.alpha_g1), beta_g2=one2(params.beta_g2), gamma_g2=one2(params.gamma_g2),
                           delta_g2=one2(params.delta_g2), gamma_abc_g1=codec.g1_from_mont(*params.gamma_abc_g1, c))


def tampered(curve, proof):
    """(2A, B, C) and (A, B, -C)"""
    G1 = Group(OC[curve], 1)
    return (groth16.Proof(G1.add(proof.a, proof.a), proof.b, proof.c), groth16.Proof(proof.a, proof.b, G1.neg(proof.c)))


def check_one(ctx, curve, params, proof, inputs, wrong_inputs):
    pvk = groth16.prepare_verifying_key(ctx, params)
    assert groth16.verify_proof(ctx, pvk, proof, inputs) is True
    assert opairing.verify_proof(OC[curve], oracle_vk(params), proof, inputs) is True          # the oracle agrees on the same proof
    for bad in tampered(curve, proof):
        assert groth16.verify_proof(ctx, pvk, bad, inputs) is False
    if wrong_inputs is not None:
        assert groth16.verify_proof(ctx, pvk, proof, wrong_inputs) is False
    for count in (len(inputs) + 1, len(inputs) - 1):
        if count >= 0:
            with pytest.raises(SynthesisError, match="MalformedVerifyingKey"):
                groth16.verify_proof(ctx, pvk, proof, [5] * count)
    return pvk


@pytest.mark.parametrize("curve", CURVES)
def test_mini_round_trip_verifies(ctx, curve):
    """x = 2, y = 3, z = 10, num = 10 (mini.rs:53-97)"""
    params = groth16.generate_parameters(ctx, curve, Mini(num=10), **TOXIC)
    pk = groth16.ProvingKey(ctx, params, Mini(num=10))
    try:
        proof = groth16.create_proof(pk, Mini(2, 3, 10, 10), 77, 88)
    finally:
        pk.free()
    pvk = check_one(ctx, curve, params, proof, [10], [11])
    vk = groth16.VerifyKey.of(params)
    assert groth16.verify_proof(ctx, groth16.prepare_verifying_key(ctx, vk), proof, [10]) is True
    assert pvk.alpha_g1_beta_g2.tolist() == groth16.prepare_verifying_key(ctx, vk).alpha_g1_beta_g2.tolist()


@pytest.mark.parametrize("curve", CURVES)
def test_mimc_chain_verifies(ctx, curve):
    """the 2^10-domain MiMC chain (1020 constraints).  The instance has no public input besides the constant one, so a WRONG public
    input cannot be formed here: that rejection runs on Mini (test_mini_round_trip_verifies) and, inside a batch, in
    test_batch_rejects_and_verify_proof_names_the_proof; here the wrong input COUNT (one input where none belongs) still raises."""
    inst = mimc_chain_instance(curve, samples_for_domain(10))
    params = groth16.generate_parameters(ctx, curve, inst, **TOXIC)
    pk = groth16.ProvingKey(ctx, params, inst)
    try:
        assert pk.domain_size == 1 << 10
        c = params.curve
        z = codec.fr_to_mont(inst.z, c).reshape(-1, 4)
        out, inf = pk.prove_raw(z, codec.fr_to_mont([0xABCDEF0123456789], c)[0], codec.fr_to_mont([0x9876543210FEDCBA], c)[0])
        proof = pk.decode_proof(out, inf)
    finally:
        pk.free()
    check_one(ctx, curve, params, proof, [], None)


@pytest.fixture(scope="module", params=CURVES)
def mini_proofs(request, ctx):
    """65 Mini proofs with distinct r, s and inputs under one key"""
    curve = request.param
    rng = random.Random(f"batch-{curve}")
    params = groth16.generate_parameters(ctx, curve, Mini(num=10), **TOXIC)
    pk = groth16.ProvingKey(ctx, params, Mini(num=10))
    proofs, inputs = [], []
    try:
        for i in range(65):
            x, y = rng.randrange(1, params.curve.r), rng.randrange(1, params.curve.r)
            z = x * (y + 2) % params.curve.r
            proofs.append(groth16.create_proof(pk, Mini(x, y, z, 10), rng.randrange(params.curve.r), rng.randrange(params.curve.r)))
            inputs.append([z])
    finally:
        pk.free()
    return curve, groth16.prepare_verifying_key(ctx, params), proofs, inputs


@pytest.mark.parametrize("n", [1, 2, 65])
def test_batch_accepts(ctx, mini_proofs, n):
    curve, pvk, proofs, inputs = mini_proofs
    assert groth16.verify_proofs_batch(ctx, pvk, proofs[:n], inputs[:n], [1] * n) is True
    assert groth16.verify_proofs_batch(ctx, pvk, proofs[:n], inputs[:n], groth16.batch_coefficients(curve, n, seed=7)) is True
    with pytest.raises(SynthesisError, match="MalformedVerifyingKey"):
        groth16.verify_proofs_batch(ctx, pvk, proofs[:n], [[1, 2]] * n, [1] * n)


def test_batch_rejects_and_verify_proof_names_the_proof(ctx, mini_proofs):
    curve, pvk, proofs, inputs = mini_proofs
    n, bad = 65, 41
    mixed = list(proofs)
    mixed[bad] = tampered(curve, proofs[bad])[0]
    for coeffs in ([1] * n, groth16.batch_coefficients(curve, n, seed=7)):
        assert groth16.verify_proofs_batch(ctx, pvk, mixed, inputs, coeffs) is False
    wrong_input = [list(x) for x in inputs]
    wrong_input[3] = [(inputs[3][0] + 1) % pvk.vk.curve.r]
    assert groth16.verify_proofs_batch(ctx, pvk, proofs, wrong_input, groth16.batch_coefficients(curve, n, seed=8)) is False
    assert [i for i in range(n) if not groth16.verify_proof(ctx, pvk, mixed[i], inputs[i])] == [bad]
