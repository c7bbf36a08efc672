"""The flow of asvc/tests/test.rs at n = 8 with fixed inputs, run through tests/asvc_ref.py, and its golden file
tests/golden/asvc_n8.json (python -m tests.asvc_cases rewrites it).  Shared by tests/test_asvc_ref.py and tests/test_gpu_asvc.py."""
import json
import random
from pathlib import Path

from oracle.pyref.curves import Group
from oracle.pyref.fields import CURVES
from tests import asvc_ref as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "asvc_n8.json"
CURVE_NAMES = ["bn254", "bls12_381"]
N = 8
TAU = 0x1234567890ABCDEF1234567890ABCDEF
G1_MULT, G2_MULT = 3, 5                      # the generators of the key as multiples of the standard ones
PROVE_POINTS = [0, 1, 5]
UPK_INDEX, UPDATE_INDEX, OTHER_INDEX = 2, 3, 4
AGG_POINTS = [1, 5]


def inputs(curve):
    c = CURVES[curve]
    rng = random.Random(f"asvc-{c.name}")
    values = [rng.randrange(c.r) for _ in range(N)]
    values[6] = c.r - 1
    return c, values, rng.randrange(1, c.r)


def generators(c):
    return Group(c, 1).mul(c.g1_gen, G1_MULT), Group(c, 2).mul(c.g2_gen, G2_MULT)


def flow(curve):
    """every point the flow produces, by name, and the parameters"""
    c, values, delta = inputs(curve)
    g1, g2 = generators(c)
    params = ref.key_gen(c, N, TAU, g1, g2)
    pk = params.proving_key
    w = ref.domain_of(c, N).group_gen
    out = {"commit": ref.commit(c, pk, values), "proof_015": ref.prove_pos(c, pk, values, PROVE_POINTS)}
    i, j = UPDATE_INDEX, OTHER_INDEX
    out["commit_updated"] = ref.update_commit(c, out["commit"], delta, i, pk.update_keys[i], w, N)
    out["proof_3"] = ref.prove_pos(c, pk, values, [i])
    out["proof_3_updated"] = ref.update_proof(c, out["proof_3"], delta, i, i, pk.update_keys[i], pk.update_keys[i], w, N)
    out["proof_4"] = ref.prove_pos(c, pk, values, [j])
    out["proof_4_updated"] = ref.update_proof(c, out["proof_4"], delta, j, i, pk.update_keys[j], pk.update_keys[i], w, N)
    singles = [ref.prove_pos(c, pk, values, [p]) for p in AGG_POINTS]
    out["proof_1"], out["proof_5"] = singles
    out["aggregate_15"] = ref.aggregate_proofs(c, N, AGG_POINTS, singles)
    return params, values, delta, out


def to_json(curve, done=None):
    _, values, delta, out = done or flow(curve)
    return {"n": N, "tau": hex(TAU), "g1_multiple": G1_MULT, "g2_multiple": G2_MULT, "values": [hex(v) for v in values],
            "delta": hex(delta), "prove_points": PROVE_POINTS, "update_index": UPDATE_INDEX, "other_index": OTHER_INDEX,
            "aggregate_points": AGG_POINTS, "points": {k: [hex(v[0]), hex(v[1])] for k, v in out.items()}}


def load_golden():
    return json.loads(GOLDEN.read_text())


def golden_points(curve):
    return {k: (int(v[0], 16), int(v[1], 16)) for k, v in load_golden()[curve]["points"].items()}


if __name__ == "__main__":
    GOLDEN.write_text(json.dumps({name: to_json(name) for name in CURVE_NAMES}, indent=1) + "\n")
    print(GOLDEN)
