"""Fused proof groups (csrc/groth16.hip ZKP_PROOF_FUSE, csrc/msm.hip `sets`): consecutive proofs of a pipelined batch share one
kernel chain — every MSM of the group is ONE MSM over several scalar vectors.  The expected value of every case is the proof of
the blocking `prove_raw`, which never fuses and which tests/test_gpu_groth16.py pins to the oracle."""
import random

import numpy as np
import pytest

from ckb_zkp_amd import codec, groth16
from ckb_zkp_amd.api import Context
from ckb_zkp_amd.circuits import MimcChain, mimc_chain_instance, samples_for_domain
from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.r1cs import ConstraintSystem
from oracle.pyref.curves import Group
from tests.util import OC, jac_limbs_to_affine_oracle, to_abi_points

pytestmark = pytest.mark.gpu
TOXIC = dict(alpha=0x1234567890ABCDEF1, beta=0xFEDCBA09876543211, gamma=0x1111111111111111111,
             delta=0x2222222222222222223, tau=0x3333333333333333335)


def _setup(ctx, curve, k):
    """-> (key, curve constants, two witnesses of the same circuit as device pointers): the instance's own and one with other
    preimages"""
    S = samples_for_domain(k)
    inst = mimc_chain_instance(curve, S, seed=0xC0FFEE)
    params = groth16.generate_parameters(ctx, curve, inst, **TOXIC)
    pk = groth16.ProvingKey(ctx, params, inst)
    c = params.curve
    assert pk.domain_size == 1 << k
    rnd = random.Random(8 + k)
    cs = ConstraintSystem(curve, True)
    MimcChain(curve, inst.constants, [(rnd.randrange(c.r), rnd.randrange(c.r)) for _ in range(S)]).generate_constraints(cs)
    zs = [codec.fr_to_mont(inst.z, c).reshape(-1, 4), codec.fr_to_mont(cs.full_assignment(), c).reshape(-1, 4)]
    return pk, c, zs


def _check_batch(ctx, pk, c, zd, order, seed):
    """a batch over the witnesses zd[order[i]] with distinct (r, s) per proof == the blocking proof of every one"""
    rnd = random.Random(seed)
    n = len(order)
    rm = codec.fr_to_mont([rnd.randrange(c.r) for _ in range(n)], c)
    sm = codec.fr_to_mont([rnd.randrange(c.r) for _ in range(n)], c)
    groups = pk.table_plan()["fused_groups"]
    out, inf = pk.prove_batch_raw([zd[j] for j in order], rm, sm)
    # the batch really ran n // 2 fused pairs (zkp_groth16_pk_info counts them, warm-up groups left out) and the remainder alone
    assert pk.table_plan()["fused_groups"] - groups == n // 2, (n, groups)
    assert out.any() or inf.all()
    for i in range(n):
        o1, i1 = pk.prove_raw(zd[order[i]], rm[i], sm[i], z_on_device=True)
        assert np.array_equal(out[i], o1) and np.array_equal(inf[i], i1), (n, i)
    return out, inf


@pytest.fixture(scope="module")
def bn_2p11(ctx):
    pk, c, zs = _setup(ctx, "bn254", 11)
    zd = [ctx.to_device(z) for z in zs]
    yield pk, c, zs, zd
    for d in zd:
        ctx.dev_free(d)
    pk.free()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17])
def test_batch_sizes(ctx, bn_2p11, n):
    """BN254 at 2^11 (1024 buckets per scalar vector: the whole pyramid inside the fused top).  3, 5 and 17 leave a remainder
    that runs as a single proof; 17 wraps the eight lanes."""
    pk, c, _, zd = bn_2p11
    _check_batch(ctx, pk, c, zd, [i % 2 for i in range(n)], seed=100 + n)


@pytest.mark.parametrize("k", [6, 13, 14])
def test_pyramid_shapes(ctx, k):
    """2^6: a tiny bucket range; 2^13: 4096 buckets per vector, one pairwise level over both vectors below the fused top and
    segmented sums of that level; 2^14: two such levels."""
    pk, c, zs = _setup(ctx, "bn254", k)
    zd = [ctx.to_device(z) for z in zs]
    try:
        _check_batch(ctx, pk, c, zd, [0, 1, 0, 1], seed=k)
    finally:
        for d in zd:
            ctx.dev_free(d)
        pk.free()


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_sets_that_differ(ctx, bn_2p11, order):
    """An ordinary witness next to one whose aux part is all zero: almost every digit of that scalar vector is dropped, so its
    buckets are empty and its L sum is the identity while the other vector's is not.  Both orders."""
    pk, c, zs, zd = bn_2p11
    z0 = zs[0].copy()
    z0[1:] = 0                                                 # the one input (the constant 1) stays
    d0 = ctx.to_device(z0)
    try:
        _check_batch(ctx, pk, c, [zd[0], d0], list(order), seed=7)
    finally:
        ctx.dev_free(d0)


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_identity_proof_points_per_proof_of_a_pair(ctx, curve):
    """Keys built as in test_identity_proof_points_through_the_host_tail: (i) the G2 side the identity everywhere, so B = O next to
    ordinary A and C in BOTH proofs of every pair; (ii) an all-identity key, A = B = C = O.  The flags and the zero limbs of each
    proof of a fused pair must come out in that proof's own slots, for two different witnesses and blinders."""
    import dataclasses

    S = 20
    inst = mimc_chain_instance(curve, S)
    params = groth16.generate_parameters(ctx, curve, inst, **TOXIC)
    c = params.curve
    rnd = random.Random(21)
    cs = ConstraintSystem(curve, True)
    MimcChain(curve, inst.constants, [(rnd.randrange(c.r), rnd.randrange(c.r)) for _ in range(S)]).generate_constraints(cs)
    zs = [codec.fr_to_mont(inst.z, c).reshape(-1, 4), codec.fr_to_mont(cs.full_assignment(), c).reshape(-1, 4)]

    def ident(q):
        return (np.zeros_like(q[0]), np.ones_like(q[1]))

    g2_off = dataclasses.replace(params, beta_g2=np.zeros_like(params.beta_g2), delta_g2=np.zeros_like(params.delta_g2),
                                 b_g2_query=ident(params.b_g2_query))
    all_off = dataclasses.replace(g2_off, alpha_g1=np.zeros_like(params.alpha_g1), beta_g1=np.zeros_like(params.beta_g1),
                                  delta_g1=np.zeros_like(params.delta_g1), a_query=ident(params.a_query),
                                  b_g1_query=ident(params.b_g1_query), h_query=ident(params.h_query),
                                  l_query=ident(params.l_query))
    fq = c.fq_limbs
    for key, flags in ((g2_off, [0, 1, 0]), (all_off, [1, 1, 1])):
        pk = groth16.ProvingKey(ctx, key, inst)
        zd = [ctx.to_device(z) for z in zs]
        try:
            out, inf = _check_batch(ctx, pk, c, zd, [0, 1, 1, 0, 0], seed=31)
        finally:
            for d in zd:
                ctx.dev_free(d)
            pk.free()
        assert inf.tolist() == [flags] * 5
        assert not out[:, 2 * fq:6 * fq].any()                              # B = O is written as zeros in every proof
        if flags[0]:
            assert not out.any()
        else:
            assert all(out[i, :2 * fq].any() and out[i, 6 * fq:].any() for i in range(5))
            assert not np.array_equal(out[0], out[1])                       # the two proofs of a pair are different proofs


def test_redo_and_chaining_under_fusion(ctx, monkeypatch):
    """Every eighth accumulate task of the fused MSMs goes through the exact redo kernel, on top of chained buckets (L -> H)."""
    monkeypatch.setenv("ZKP_DEBUG_FORCE_REDO", "1")
    x = Context(ctx.device)                                    # latches the switch
    monkeypatch.delenv("ZKP_DEBUG_FORCE_REDO")
    pk = None
    zd = []
    try:
        pk, c, zs = _setup(x, "bn254", 11)
        zd = [x.to_device(z) for z in zs]
        _check_batch(x, pk, c, zd, [0, 1, 0, 1], seed=4)
    finally:
        for d in zd:
            x.dev_free(d)
        if pk:
            pk.free()
        x.close()


def test_second_curve(ctx):
    """BLS12-381 at 2^9: twelve-limb coordinates, the saturated-layout G2 path."""
    pk, c, zs = _setup(ctx, "bls12_381", 9)
    zd = [ctx.to_device(z) for z in zs]
    try:
        _check_batch(ctx, pk, c, zd, [0, 1, 0, 1], seed=9)
    finally:
        for d in zd:
            ctx.dev_free(d)
        pk.free()


@pytest.mark.parametrize("log_n", [12, 13])
def test_single_msm_is_unchanged(ctx, log_n):
    """One scalar vector is the plain MSM: a stand-alone G1 MSM against the C++ oracle's Pippenger and the known discrete log."""
    from oracle import cpu_oracle
    curve, group = "bn254", 1
    c = get_curve(curve)
    G = Group(OC[curve], group)
    n = (1 << log_n) + 5
    rng = np.random.default_rng(40 + log_n)
    d = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    d[:, 3] >>= np.uint64(4)
    g_xy, _ = to_abi_points(curve, group, [G.gen])
    xy, inf = cpu_oracle.fixed_base_mul(c.cid, group, g_xy, d)
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)          # < r
    bases = ctx.upload_bases(c, group, xy, inf)
    try:
        got = jac_limbs_to_affine_oracle(curve, group, bases.msm(k))
        assert got == jac_limbs_to_affine_oracle(curve, group, cpu_oracle.msm(c.cid, group, xy, inf, k, threads=8))
        e = sum(a * b for a, b in zip(codec.limbs_to_ints(d), codec.limbs_to_ints(k))) % c.r
        assert got == G.mul(G.gen, e)
    finally:
        bases.free()
