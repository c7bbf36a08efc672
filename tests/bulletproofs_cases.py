"""Circuits, generators, randomness and the transcript stand-in shared by the Bulletproofs tests (tests/test_bulletproofs_ref.py,
tests/test_gpu_bulletproofs.py), and the golden proof of the reference's `mini` circuit.

    python -m tests.bulletproofs_cases        rewrites tests/golden/bulletproofs_mini.json from tests/bulletproofs_ref.py
"""
import hashlib
import json
from pathlib import Path

import numpy as np

from ckb_zkp_amd import codec
from ckb_zkp_amd.bulletproofs import Generators
from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.r1cs import ConstraintSystem
from tests.gkr_cases import rand_fr

GOLDEN = Path(__file__).resolve().parent / "golden" / "bulletproofs_mini.json"
MINI_CURVE, MINI_SEED = "bls12_381", 381


def mini(curve, z=10):
    """bulletproofs/tests/mini.rs: x (y + 2) = z ten times with x = 2, y = 3; aux x, y and the input z: n = 10, n_w = 2, N = 16"""
    cs = ConstraintSystem(curve, assign=True)
    var_x = cs.alloc(lambda: 2)
    var_y = cs.alloc(lambda: 3)
    var_z = cs.alloc_input(lambda: z)
    for _ in range(10):
        cs.enforce(lambda lc: lc + var_x, lambda lc: lc + var_y + (2, cs.one()), lambda lc: lc + var_z)
    return cs


def random_circuit(curve, n, n_w, seed, num_public=1):
    """a satisfied system of n constraints over n_w aux variables and 1 + num_public inputs: two random sparse rows and a third
    one, over the one and an aux variable, that makes the product hold"""
    c = get_curve(curve)
    r = c.r
    rng = np.random.default_rng(seed)
    cs = ConstraintSystem(curve, assign=True)
    vals = rand_fr(r, n_w + num_public, seed + 1)
    pub = [cs.alloc_input(lambda v=v: v) for v in vals[:num_public]]
    aux = [cs.alloc(lambda v=v: v) for v in vals[num_public:]]
    variables = [cs.one()] + pub + aux
    f = cs.full_assignment()                                      # inputs ++ aux, the order of `variables`
    coeffs = iter(rand_fr(r, 8 * n, seed + 2))
    for i in range(n):
        rows = []
        for _ in range(2):
            picks = rng.choice(len(variables), size=min(3, len(variables)), replace=False)
            rows.append([(next(coeffs), int(j)) for j in picks])
        a_val, b_val = (sum(k * f[j] for k, j in row) % r for row in rows)
        j = 1 + num_public + i % n_w                              # every aux column occurs when n >= n_w
        c2 = next(coeffs)
        c1 = (a_val * b_val - c2 * f[j]) % r
        rows.append([(c1, 0), (c2, j)])
        cs.enforce(*[(lambda lc, row=row: _extend(lc, row, variables)) for row in rows])
    return cs


def _extend(lc, row, variables):
    for k, j in row:
        lc = lc + (k, variables[j])
    return lc


def generators(curve, N, seed):
    """(integer points (g_vec, h_vec, g, h, u), the same as a Generators of Montgomery arrays)"""
    from tests.bulletproofs_ref import group
    c = get_curve(curve)
    G = group(c)
    pts = [G.mul(G.gen, k or 1) for k in rand_fr(c.r, 2 * N + 3, seed)]
    xy, inf = codec.g1_to_mont(pts, c)
    assert not inf.any()
    ints = (pts[:N], pts[N:2 * N], pts[2 * N], pts[2 * N + 1], pts[2 * N + 2])
    return ints, Generators(xy[:N], xy[N:2 * N], xy[2 * N], xy[2 * N + 1], xy[2 * N + 2])


def randomness(curve, cs, seed):
    """the 2 max(n, n_w) + 12 values the prover draws"""
    return rand_fr(get_curve(curve).r, 2 * max(cs.num_constraints(), cs.num_aux) + 12, seed)


class Challenger:
    """SHA-256 over everything sent so far: every challenge absorbs the state before it and the message at hand"""

    def __init__(self, curve, tag=b"bulletproofs"):
        self.r = get_curve(curve).r
        self.state = hashlib.sha256(tag).digest()

    def _next(self, label, data):
        self.state = hashlib.sha256(self.state + label + data).digest()
        return int.from_bytes(hashlib.sha256(self.state + b"challenge").digest() + self.state, "little") % self.r or 1

    @staticmethod
    def _points(pts):
        return b"".join(np.ascontiguousarray(xy, dtype=np.uint64).tobytes() + bytes([1 if inf else 0]) for xy, inf in pts)

    def yz(self, a_i, a_o, a_w, s):
        data = self._points([a_i, a_o, a_w, s])
        return self._next(b"y", data), self._next(b"z", b"")

    def x(self, t_points):
        return self._next(b"x", self._points(t_points))

    def x1(self, t_x, tau_x, mu, l_x, r_x):
        data = b"".join(int(v).to_bytes(32, "little") for v in (t_x, tau_x, mu))
        return self._next(b"x_1", data + np.ascontiguousarray(l_x).tobytes() + np.ascontiguousarray(r_x).tobytes())

    def ipa(self, l_pt, r_pt):
        return self._next(b"ipa", self._points([l_pt, r_pt]))


def same_point(p, q):
    return bool(p[1]) == bool(q[1]) and np.array_equal(np.asarray(p[0], dtype=np.uint64), np.asarray(q[0], dtype=np.uint64))


def assert_same_proof(p, q):
    """field for field; every group element is affine, so equality is bitwise"""
    for name in ("A_I", "A_O", "A_W", "S", "IPP_P"):
        assert same_point(getattr(p, name), getattr(q, name)), name
    for name in ("T", "L_vec", "R_vec"):
        a, b = getattr(p, name), getattr(q, name)
        assert len(a) == len(b) and all(same_point(s, t) for s, t in zip(a, b)), name
    for name in ("mu", "tau_x", "t_x", "a", "b"):
        assert getattr(p, name) == getattr(q, name), name
    assert np.array_equal(p.l_x, q.l_x) and np.array_equal(p.r_x, q.r_x)


def proof_to_json(proof, curve):
    c = get_curve(curve)
    pt = lambda p: None if p[1] else [str(v) for v in codec.g1_from_mont(np.asarray(p[0]).reshape(1, -1), None, c)[0]]   # noqa: E731
    return {"curve": c.name, "seed": MINI_SEED,
            **{k: pt(getattr(proof, k)) for k in ("A_I", "A_O", "A_W", "S", "IPP_P")},
            **{k: [pt(p) for p in getattr(proof, k)] for k in ("T", "L_vec", "R_vec")},
            **{k: str(getattr(proof, k)) for k in ("mu", "tau_x", "t_x", "a", "b")},
            "l_x": [str(v) for v in codec.fr_from_mont(proof.l_x, c)], "r_x": [str(v) for v in codec.fr_from_mont(proof.r_x, c)]}


def load_golden():
    return json.loads(GOLDEN.read_text())


def mini_setup(curve, seed=MINI_SEED):
    """(cs, integer generators, Generators, randomness) of the mini proof"""
    cs = mini(curve)
    ints, gens = generators(curve, 16, seed)
    return cs, ints, gens, randomness(curve, cs, seed + 1)


if __name__ == "__main__":
    from tests import bulletproofs_ref as ref
    cs_, ints_, _, rand_ = mini_setup(MINI_CURVE)
    proof_ = ref.prove(MINI_CURVE, cs_, ints_, rand_, Challenger(MINI_CURVE))
    assert ref.verify(MINI_CURVE, cs_, ints_, proof_, [10], Challenger(MINI_CURVE))
    GOLDEN.write_text(json.dumps(proof_to_json(proof_, MINI_CURVE), indent=1) + "\n")
    print(GOLDEN)
