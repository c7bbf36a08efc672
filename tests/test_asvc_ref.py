"""CPU: tests/asvc_ref.py, the Python-integer restatement of asvc/src/lib.rs, on the flow of asvc/tests/test.rs at n = 8, both curves.
The reference cannot be built here (no cargo), so parity stays unpinned by the reference (oracle/README.md): what is pinned is that
the restated verifiers accept what the restated provers produce and reject tampered inputs, that a proof is [q(tau)] g1, that the
partial-fraction identity the device kernel rests on reproduces long division, and the golden file."""
import random

import pytest

from oracle.pyref.curves import Group
from tests import asvc_cases as cases
from tests import asvc_ref as ref

CURVES = cases.CURVE_NAMES


@pytest.fixture(scope="module")
def flows():
    return {name: cases.flow(name) for name in CURVES}


@pytest.mark.parametrize("curve", CURVES)
def test_flow_verifies_and_rejects_tampering(flows, curve):
    params, values, delta, out = flows[curve]
    c = cases.inputs(curve)[0]
    vk, pk = params.verification_key, params.proving_key
    w = ref.domain_of(c, cases.N).group_gen
    G1 = Group(c, 1)
    pts = cases.PROVE_POINTS
    vals = [values[p] for p in pts]
    assert ref.verify_pos(c, vk, out["commit"], vals, pts, out["proof_015"], w)
    assert not ref.verify_pos(c, vk, out["commit"], [vals[0] + 1] + vals[1:], pts, out["proof_015"], w)          # a tampered value
    assert not ref.verify_pos(c, vk, out["commit"], vals, pts, G1.add(out["proof_015"], c.g1_gen), w)            # a tampered proof
    assert not ref.verify_pos(c, vk, out["commit"], vals, [0, 1, 6], out["proof_015"], w)                        # a tampered position
    assert ref.verify_upk(c, vk, cases.UPK_INDEX, pk.update_keys[cases.UPK_INDEX], w)
    assert not ref.verify_upk(c, vk, cases.UPK_INDEX, pk.update_keys[cases.UPK_INDEX + 1], w)
    i, j = cases.UPDATE_INDEX, cases.OTHER_INDEX
    assert ref.verify_pos(c, vk, out["commit_updated"], [(values[i] + delta) % c.r], [i], out["proof_3_updated"], w)
    assert not ref.verify_pos(c, vk, out["commit_updated"], [values[i]], [i], out["proof_3"], w)
    assert ref.verify_pos(c, vk, out["commit_updated"], [values[j]], [j], out["proof_4_updated"], w)
    agg = cases.AGG_POINTS
    assert ref.verify_pos(c, vk, out["commit"], [values[p] for p in agg], agg, out["aggregate_15"], w)
    assert out["aggregate_15"] == ref.prove_pos(c, pk, values, agg)


@pytest.mark.parametrize("curve", CURVES)
def test_proof_is_the_quotient_at_tau_in_the_exponent(flows, curve):
    params, values, _, out = flows[curve]
    c = cases.inputs(curve)[0]
    g1, _ = cases.generators(c)
    assert out["proof_015"] == ref.prove_pos_in_exponent(c, cases.N, cases.TAU, g1, values, cases.PROVE_POINTS)
    assert out["commit"] == Group(c, 1).mul(g1, sum(v * l for v, l in zip(values, params.scalars["l"])) % c.r)
    # all n positions: the quotient is empty, the proof the identity
    assert ref.prove_pos(c, params.proving_key, values, list(range(cases.N))) is None


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [8, 16, 64])
def test_identity_reproduces_long_division(curve, n):
    c = cases.inputs(curve)[0]
    rng = random.Random(n)
    phi = [rng.randrange(c.r) for _ in range(n)]
    for k in (1, 2, 3, 5, n - 1, n):
        points = rng.sample(range(n), k)
        q = ref.quotient(c, phi, points)
        by_identity = ref.quotient_by_identity(c, phi, points)
        assert len(q) == n - k
        assert by_identity[:n - k] == q and not any(by_identity[n - k:])
        assert ref.subset_weights(c, n, points) == ref.subset_weights_direct(c, n, points)
    assert ref.subset_weights(c, n, [3]) == [1]


def test_golden_file_matches_the_ref(flows):
    golden = cases.load_golden()
    for curve in CURVES:
        assert golden[curve] == cases.to_json(curve, flows[curve])
        assert cases.golden_points(curve) == flows[curve][3]
