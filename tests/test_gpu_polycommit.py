"""ckb_zkp_amd.polycommit on the device against tests/polycommit_ref.py (Python integers): packing_poly_commit and reduce_prover
at s = 4 (4 x 4), 5 (4 x 8, the uneven split) and 8 (16 x 16), blind and not blind, both curves.  Under the same `rand` and
challenger the commitments and the proof are equal bit for bit; the reference verifier accepts the device's proof and rejects it
when the polynomial is changed after the commitment; a vector of length 1 gives zero rounds."""
import random

import numpy as np
import pytest

from ckb_zkp_amd import polycommit as pc
from ckb_zkp_amd.params import get_curve
from tests import polycommit_ref as ref
from tests.bulletproofs_ref import abi_point, int_point

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]


@pytest.fixture(scope="module")
def params(ctx):
    made = {}

    def get(curve, s):
        if (curve, s) not in made:
            made[(curve, s)] = pc.setup(ctx, curve, s, f"polycommit {curve} {s}")
        return made[(curve, s)]
    yield get
    for p in made.values():
        p.free()


def case(c, s, is_blind):
    rng = random.Random(f"gpu polycommit {c.name} {s} {is_blind}")
    l_size, r_size = pc.split_sizes(s)
    poly = [rng.randrange(c.r) for _ in range(1 << s)]
    ry = [rng.randrange(c.r) for _ in range(s)]
    ev = ref.dot(ref.eval_eq(ry, c.r), poly, c.r)
    rand_commit = [rng.randrange(c.r) for _ in range(l_size)] if is_blind else []
    rand_open = [rng.randrange(c.r) for _ in range(3 + 2 * ref.log2(r_size))]
    return poly, ry, ev, rand_commit, rand_open, (rng.randrange(c.r) if is_blind else 0)


@pytest.mark.parametrize("is_blind", [False, True])
@pytest.mark.parametrize("s", [4, 5, 8])
@pytest.mark.parametrize("curve", CURVES)
def test_commit_and_open_match_the_reference(params, curve, s, is_blind):
    c = get_curve(curve)
    P = params(curve, s)
    R = ref.RefParams.of(P)
    assert P.n == pc.split_sizes(s)[1] == R.n
    poly, ry, ev, rand_commit, rand_open, ry_blind = case(c, s, is_blind)
    comms, blinds = pc.packing_poly_commit(P, poly, rand_commit, is_blind)
    want_comms, want_blinds = ref.packing_poly_commit(R, poly, rand_commit, is_blind)
    assert blinds == want_blinds and len(comms) == pc.split_sizes(s)[0]
    assert all(ref.same_point(a, abi_point(b, c)) for a, b in zip(comms, want_comms))
    # a device-resident polynomial gives the same commitments and the same proof
    dev = pc.DevicePoly(P.ctx, c, poly)
    try:
        comms_dev, _ = pc.packing_poly_commit(P, dev, rand_commit, is_blind)
        assert all(ref.same_point(a, b) for a, b in zip(comms, comms_dev))
        ch = ref.HashChallenger(c)
        proof, comm_y = pc.reduce_prover(P, dev, blinds if is_blind else [], ry, ry_blind, ev, rand_open, ch)
    finally:
        dev.free()
    proof2, comm_y2 = pc.reduce_prover(P, poly, blinds if is_blind else [], ry, ry_blind, ev, rand_open, ref.HashChallenger(c))
    assert ref.same_proof(proof, proof2) and ref.same_point(comm_y, comm_y2)
    k = ref.log2(P.n)
    assert ch.log == ["Cx", "Cy"] + ["L", "R", "x"] * k + ["delta", "beta", "c"]
    want_proof, want_y = ref.reduce_prover(R, poly, blinds if is_blind else [], ry, ry_blind, ev, rand_open, ref.HashChallenger(c))
    assert ref.same_point(comm_y, abi_point(want_y, c))
    assert ref.same_proof(proof, ref.proof_to_abi(want_proof, c))
    # the reference verifier: accepts; rejects once the polynomial is changed after the commitment
    int_comms = [int_point(p, c) for p in comms]
    assert ref.reduce_verifier(R, ref.proof_to_int(proof, c), ry, int_comms, int_point(comm_y, c), ref.HashChallenger(c))
    bad = list(poly)
    bad[len(bad) // 3] = (bad[len(bad) // 3] + 1) % c.r
    bad_proof, bad_y = pc.reduce_prover(P, bad, blinds if is_blind else [], ry, ry_blind, ev, rand_open, ref.HashChallenger(c))
    assert not ref.reduce_verifier(R, ref.proof_to_int(bad_proof, c), ry, int_comms, int_point(bad_y, c), ref.HashChallenger(c))


@pytest.mark.parametrize("curve", CURVES)
def test_poly_commit_vec_and_length_one(params, curve):
    c = get_curve(curve)
    P = params(curve, 4)
    R = ref.RefParams.of(P)
    rng = random.Random("vec " + curve)
    for n in (1, 3, P.n):                                            # rows = 1, cols <= n
        vals, blind = [rng.randrange(c.r) for _ in range(n)], rng.randrange(c.r)
        assert ref.same_point(pc.poly_commit_vec(P, vals, blind), abi_point(ref.poly_commit_vec(R, R.gens, vals, R.h, blind), c))
    rand = [rng.randrange(c.r) for _ in range(3)]
    x, a, bx, by = rng.randrange(c.r), rng.randrange(c.r), rng.randrange(c.r), rng.randrange(c.r)
    proof, cx, cy = pc.log_dot_product_prove(P, [x], bx, [a], x * a % c.r, by, rand, ref.HashChallenger(c))
    assert proof[0] == [] and proof[1] == []                         # zero rounds
    want, wx, wy = ref.log_dot_product_prove(R, [x], bx, [a], x * a % c.r, by, rand, ref.HashChallenger(c))
    assert ref.same_proof(proof, ref.proof_to_abi(want, c)) and ref.same_point(cx, abi_point(wx, c)) and ref.same_point(cy, abi_point(wy, c))
    assert ref.log_dot_product_verify(R, ref.proof_to_int(proof, c), int_point(cx, c), int_point(cy, c), [a], ref.HashChallenger(c))
    with pytest.raises(ValueError):                                  # the prover draws exactly 3 + 2 log2(n) values
        pc.log_dot_product_prove(P, [x], bx, [a], x * a % c.r, by, rand + [1], ref.HashChallenger(c))
    assert isinstance(np.asarray(cx[0]), np.ndarray)
