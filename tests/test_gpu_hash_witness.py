"""hashes.mimc_chain_witness_dev: the witness of the headline circuit written on the device equals
circuits.mimc_chain_instance(...).z bit for bit, and the Groth16 proof over it equals the proof from the host witness."""
import numpy as np
import pytest

from ckb_zkp_amd import codec, groth16, hashes
from ckb_zkp_amd.circuits import MIMC_ROUNDS, mimc_chain_instance, samples_for_domain
from ckb_zkp_amd.params import get_curve

pytestmark = pytest.mark.gpu
TOXIC = dict(alpha=0x1234567890ABCDEF1, beta=0xFEDCBA09876543211, gamma=0x1111111111111111111,
             delta=0x2222222222222222223, tau=0x3333333333333333335)
SENT = 0xDEADBEEFCAFEF00D


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_device_witness_equals_the_host_witness_and_gives_the_same_proof(ctx, curve):
    c = get_curve(curve)
    S = samples_for_domain(10)
    inst = mimc_chain_instance(curve, S)
    want = codec.fr_to_mont(inst.z, c).reshape(-1, 4)
    assert want.shape[0] == 1 + (2 * MIMC_ROUNDS + 2) * S
    params = hashes.HashParams.mimc(ctx, curve, inst.constants)
    pre = [xl for xl, _ in inst.preimages] + [xr for _, xr in inst.preimages]
    sent = np.full((1, 4), SENT, dtype=np.uint64)
    host_pre = np.concatenate([sent, codec.fr_to_mont(pre, c), sent])
    d_pre = ctx.to_device(host_pre)
    z_dev, pk = 0, None
    try:
        z_dev = hashes.mimc_chain_witness_dev(ctx, params, d_pre + 32, S)
        ctx.sync()
        got, got_pre = np.zeros_like(want), np.zeros_like(host_pre)
        ctx.d2h(got, z_dev)
        ctx.d2h(got_pre, d_pre)
        assert np.array_equal(got_pre, host_pre), "the pre-images changed"
        assert np.array_equal(got, want)
        pk = groth16.ProvingKey(ctx, groth16.generate_parameters(ctx, curve, inst, **TOXIC), inst)
        assert pk.domain_size == 1 << 10
        r, s = codec.fr_to_mont([0x1357, 0x2468ACE], c)
        from_host = pk.prove_raw(want, r, s)
        from_dev = pk.prove_raw(z_dev, r, s, z_on_device=True)
        assert np.array_equal(from_host[0], from_dev[0]) and np.array_equal(from_host[1], from_dev[1])
        assert from_dev[0].any()
    finally:
        if pk:
            pk.free()
        if z_dev:
            ctx.dev_free(z_dev)
        ctx.dev_free(d_pre)
        params.free()
    with pytest.raises(ValueError):                                 # the chain is MiMC-5
        hashes.mimc_chain_witness_dev(ctx, hashes.HashParams(ctx, curve, hashes.KIND_MIMC, 4, 0), 0, 1)
