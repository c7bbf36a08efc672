"""sha256.witness_dev on the device: the assignment of a synthesised bit circuit written from its messages alone, element for
element equal to the host synthesis, and a Groth16 proof from that resident assignment.

Sha256Block (512 + 25 840 constraints, domain 2^15) on both curves; on BN254 its proof from the device z equals the proof from
the host z, and groth16.verify_proof accepts it.  The circuit has the shape of the reference's test_full_block: its 512 bits are
auxiliary variables, so its only input is the constant one and there is no public input to flip.  The rejection is therefore
checked on what the proof does bind: a proof made from the same z with one bit flipped is refused, and so is a public input
where the key expects none.  Sha256Merkle at depth 2, a left and a right index, two instances with different leaves: z equality
only.  Each circuit is synthesised once per module."""
import functools
import random

import numpy as np
import pytest

from ckb_zkp_amd import circuits, codec, groth16, merkle
from ckb_zkp_amd import sha256 as S
from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.r1cs import R1csInstance, SynthesisError
from tests import sha256_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
TOXIC = dict(alpha=0x1234567890ABCDEF1, beta=0xFEDCBA09876543211, gamma=0x1111111111111111111,
             delta=0x2222222222222222223, tau=0x3333333333333333335)


@functools.lru_cache(maxsize=None)
def block(curve):
    c = circuits.Sha256Block([random.Random(77).getrandbits(1) for _ in range(512)])
    return (c,) + S.synthesize(c, curve, True)


@functools.lru_cache(maxsize=None)
def membership(curve, leaf_index):
    """two instances of one shape: the same index in two trees of four leaves"""
    out = []
    for seed in (1, 2):
        rng = random.Random(10 * seed + leaf_index)
        leaves = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(4)]
        nodes = ref.cbmt(leaves)
        lemmas = ref.cbmt_proof(nodes, leaf_index)
        c = circuits.Sha256Merkle(3 + leaf_index, leaves[leaf_index], lemmas, nodes[0])
        cs, plan = S.synthesize(c, curve, True)
        out.append((cs, plan, merkle.membership_messages(3 + leaf_index, leaves[leaf_index], lemmas)))
    return out


def device_z(ctx, curve, plan, msgs, q, gap=0):
    """witness_dev -> (q, len + gap, 4) Montgomery words"""
    flat = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    d_m, pd = ctx.to_device(flat), S.upload_plan(ctx, plan)
    m = len(plan.codes)
    try:
        z_dev = S.witness_dev(ctx, curve, pd, d_m, q, m + gap)
        try:
            got = np.zeros((q, m + gap, 4), dtype=np.uint64)
            ctx.d2h(got, z_dev)
        finally:
            ctx.dev_free(z_dev)
    finally:
        pd.free()
        ctx.dev_free(d_m)
    return got


@pytest.mark.parametrize("curve", CURVES)
def test_block_witness_equals_the_host_assignment(ctx, curve):
    c, cs, plan = block(curve)
    assert cs.num_constraints() == 512 + 25840 and 1 << 14 < cs.num_constraints() + 1 <= 1 << 15
    got = device_z(ctx, curve, plan, c.message_bytes(), 1)
    assert np.array_equal(got[0], codec.fr_to_mont(cs.full_assignment(), get_curve(curve)))


def test_block_proof_from_the_device_assignment(ctx):
    curve = "bn254"
    cv = get_curve(curve)
    c, cs, plan = block(curve)
    inst = R1csInstance.from_cs(cs)
    params = groth16.generate_parameters(ctx, curve, inst, **TOXIC)
    pk = groth16.ProvingKey(ctx, params, inst)
    d_m, pd = ctx.to_device(np.frombuffer(c.message_bytes()[0], dtype=np.uint8)), S.upload_plan(ctx, plan)
    z_dev = 0
    try:
        assert pk.domain_size == 1 << 15
        z_host = codec.fr_to_mont(cs.full_assignment(), cv)
        rm, sm = codec.fr_to_mont([0x5EED], cv)[0], codec.fr_to_mont([0xFACE], cv)[0]
        z_dev = S.witness_dev(ctx, curve, pd, d_m, 1)
        out_d, inf_d = pk.prove_raw(z_dev, rm, sm, z_on_device=True)
        out_h, inf_h = pk.prove_raw(z_host, rm, sm)
        assert np.array_equal(out_d, out_h) and np.array_equal(inf_d, inf_h)
        proof = pk.decode_proof(out_d, inf_d)
        pvk = groth16.prepare_verifying_key(ctx, params)
        assert groth16.verify_proof(ctx, pvk, proof, [])
        with pytest.raises(SynthesisError):
            groth16.verify_proof(ctx, pvk, proof, [1])                                      # the key expects no public input
        bad = z_host.copy()
        j = 1 + 512 + 100                                                                   # a computed bit
        bad[j] = codec.fr_mont(1 - cs.full_assignment()[j], cv)
        out_b, inf_b = pk.prove_raw(bad, rm, sm)
        assert not groth16.verify_proof(ctx, pvk, pk.decode_proof(out_b, inf_b), [])
    finally:
        if z_dev:
            ctx.dev_free(z_dev)
        pd.free()
        ctx.dev_free(d_m)
        pk.free()


@pytest.mark.parametrize("leaf_index", [0, 1])
@pytest.mark.parametrize("curve", CURVES)
def test_membership_witness_of_two_instances(ctx, curve, leaf_index):
    (cs0, plan0, msgs0), (cs1, plan1, msgs1) = membership(curve, leaf_index)
    assert plan0 == plan1 and plan0.messages == 2 and msgs0 != msgs1 and cs0.full_assignment() != cs1.full_assignment()
    got = device_z(ctx, curve, plan0, msgs0 + msgs1, 2, gap=5)
    cv = get_curve(curve)
    m = len(plan0.codes)
    for b, cs in enumerate((cs0, cs1)):
        assert np.array_equal(got[b, :m], codec.fr_to_mont(cs.full_assignment(), cv)), b
