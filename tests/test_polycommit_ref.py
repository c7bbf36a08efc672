"""CPU: tests/polycommit_ref.py is consistent with itself — the verifier accepts the reference prover's proof and rejects it after
one matrix element, eval, z1 or one L point is changed, and lz equals the direct evaluation sum_k eq(ry)[k] poly[k] folded with R.
Both curves, s = 4 (4 x 4) and s = 5 (4 x 8, the uneven split).  Parity with the Rust reference is unpinned: it cannot be built
here (see the module's docstring)."""
import random

import pytest

from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.polycommit import split_sizes
from tests import polycommit_ref as ref

CURVES = ["bn254", "bls12_381"]


def make_case(curve, s, is_blind, seed=0):
    c = get_curve(curve)
    rng = random.Random(f"polycommit {curve} {s} {is_blind} {seed}")
    G = ref.group(c)
    l_size, r_size = split_sizes(s)
    pts = [G.mul(G.gen, rng.randrange(1, c.r)) for _ in range(r_size + 2)]
    P = ref.RefParams(c, pts[:r_size], pts[r_size], pts[r_size + 1])
    poly = [rng.randrange(c.r) for _ in range(1 << s)]
    ry = [rng.randrange(c.r) for _ in range(s)]
    eq = ref.eval_eq(ry, c.r)
    ev = ref.dot(eq, poly, c.r)
    rand_commit = [rng.randrange(c.r) for _ in range(l_size)]
    rand_open = [rng.randrange(c.r) for _ in range(3 + 2 * ref.log2(r_size))]
    ry_blind = rng.randrange(c.r) if is_blind else 0
    return c, P, poly, ry, ev, rand_commit, rand_open, ry_blind


def prove(c, P, poly, ry, ev, rand_commit, rand_open, ry_blind, is_blind):
    comms, blinds = ref.packing_poly_commit(P, poly, rand_commit if is_blind else [], is_blind)
    proof, comm_y = ref.reduce_prover(P, poly, blinds if is_blind else [], ry, ry_blind, ev, rand_open, ref.HashChallenger(c))
    return comms, proof, comm_y


@pytest.mark.parametrize("is_blind", [False, True])
@pytest.mark.parametrize("s", [4, 5])
@pytest.mark.parametrize("curve", CURVES)
def test_verifier_accepts_and_rejects(curve, s, is_blind):
    c, P, poly, ry, ev, rand_commit, rand_open, ry_blind = make_case(curve, s, is_blind)
    assert split_sizes(s) == ((4, 4) if s == 4 else (4, 8))
    comms, proof, comm_y = prove(c, P, poly, ry, ev, rand_commit, rand_open, ry_blind, is_blind)
    assert len(comms) == split_sizes(s)[0] and len(proof[0]) == len(proof[1]) == ref.log2(split_sizes(s)[1])
    ch = ref.HashChallenger(c)
    assert ref.reduce_verifier(P, proof, ry, comms, comm_y, ch)
    k = len(proof[0])
    assert ch.log == ["Cx", "Cy"] + ["L", "R", "x"] * k + ["delta", "beta", "c"]      # the reference's labels in its order
    verify = lambda pr, cm, cy: ref.reduce_verifier(P, pr, ry, cm, cy, ref.HashChallenger(c))
    # one matrix element changed after the commitment
    bad = list(poly)
    bad[5] = (bad[5] + 1) % c.r
    blinds = [b % c.r for b in rand_commit] if is_blind else []                       # the blinds of the commitment, row by row
    bad_proof, bad_y = ref.reduce_prover(P, bad, blinds, ry, ry_blind, ev, rand_open, ref.HashChallenger(c))
    assert not verify(bad_proof, comms, bad_y)
    # eval changed: the prover's comm_y no longer opens to the claimed value
    wrong_y = ref.poly_commit_vec(P, [P.g1], [(ev + 1) % c.r], P.h, ry_blind)
    assert not verify(proof, comms, wrong_y)
    l_vec, r_vec, delta, beta, z1, z2 = proof
    assert not verify((l_vec, r_vec, delta, beta, (z1 + 1) % c.r, z2), comms, comm_y)
    assert not verify(([P.G.add(l_vec[0], P.g1)] + l_vec[1:], r_vec, delta, beta, z1, z2), comms, comm_y)


@pytest.mark.parametrize("s", [4, 5])
@pytest.mark.parametrize("curve", CURVES)
def test_row_fold_is_the_evaluation(curve, s):
    c, P, poly, ry, ev, *_ = make_case(curve, s, False, seed=1)
    lz, l_eq, r_eq = ref.row_fold(poly, ry, c.r)
    assert ref.dot(lz, r_eq, c.r) == ev
    l_size, r_size = split_sizes(s)
    full = ref.eval_eq(ry, c.r)
    assert all(full[i * r_size + j] == l_eq[i] * r_eq[j] % c.r for i in range(l_size) for j in range(r_size))
    assert sum(full) % c.r == 1
    # eq(., ry) at a corner: ry = bits of idx selects poly[idx]; ry[0] is the most significant bit
    idx = 0b1011 if s == 4 else 0b10110
    bits = [(idx >> (s - 1 - i)) & 1 for i in range(s)]
    assert ref.dot(ref.eval_eq(bits, c.r), poly, c.r) == poly[idx]


def test_length_one_has_zero_rounds():
    c, P, *_ = make_case("bn254", 4, False)
    proof, cx, cy = ref.log_dot_product_prove(P, [7], 3, [5], 35, 4, [11, 12, 13], ref.HashChallenger(c))
    assert proof[0] == [] and proof[1] == []
    assert ref.log_dot_product_verify(P, proof, cx, cy, [5], ref.HashChallenger(c))
    assert not ref.log_dot_product_verify(P, proof, cx, ref.poly_commit_vec(P, [P.g1], [36], P.h, 4), [5], ref.HashChallenger(c))
