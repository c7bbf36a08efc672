"""The small group entry points against the Python curve (oracle/pyref: affine chord-and-tangent and its scalar multiplication):
zkp_g1/g2_fold, zkp_g1/g2_into_affine, zkp_fixed_base_mul_g1/g2, zkp_groth16_assemble and zkp_groth16_fold_assemble_dev, on both
curves.  Every input is built HERE from affine points of known discrete log and a chosen Z (X = x Z^2, Y = y Z^3, Montgomery
words; XYZZ slots as (x z^2, y z^3, z^2, z^3)); every result is decoded here with integers.  No device call makes an input or
an expected value, and cpu_oracle (a port of the same formulas) is not the reference.

The scalars of the assembly tests come from EDGE: {0, 1, 2, r-1, lambda, lambda+1, r-lambda} and tests/glv_ref.GLV_EDGE, the
scalars the CPU run of the shipped split (tests/test_glv_split.py) selects: largest |k1| and |k2|, k1 = 0, k2 = 0, and each
reachable sign pair — on BN254 that includes the one-in-2^63 scalar with k2 < 0.

Reference of the assembly (zkp_accel.h; ckb_zkp_amd/distributed.py ShardedGroth16Prover, which folds alpha, beta, delta r, delta s
and -rs delta into the five sums; the reference prover's groth16/src/prover.rs:192-210 as quoted in msm_group.hip): with
A = a G, B1 = b1 G, B2 = b2 G2, H = h G, L = l G
    proof.a = A,   proof.b = B2,   proof.c = (s a + r b1 + h + l) G.

Measured on an MI355X: the whole file (20 tests) takes 5.7 s; the slowest test (the 121 (r, s) pairs of the assembly on
BLS12-381) 0.9 s, an assembly call about 1 ms; the Python curve arithmetic is most of the rest.
"""
import random
import time

import numpy as np
import pytest

from ckb_zkp_amd import codec, groth16
from ckb_zkp_amd.params import get_curve
from oracle.pyref.curves import Group
from tests import glv_ref
from tests.util import OC

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
CG = [(cv, g) for cv in CURVES for g in (1, 2)]


# ------------------------------------------------------------------------------------------------------------ encoding
class Enc:
    """Field elements (ints / (c0, c1) tuples of oracle/pyref) <-> Montgomery uint64 limbs of group `g` on `curve`."""

    def __init__(self, curve, g):
        self.c, self.g = get_curve(curve), g
        self.G = Group(OC[curve], g)
        self.Fo = self.G.F
        self.f = self.c.fq_limbs
        self.R = 1 << (64 * self.f)
        self.Ri = pow(self.R, -1, self.c.q)

    def comps(self, e):
        return (e,) if self.g == 1 else tuple(e)

    def limbs(self, *elts) -> np.ndarray:
        return codec.ints_to_limbs([v * self.R % self.c.q for e in elts for v in self.comps(e)], self.f).reshape(-1)

    def elts(self, words, n):
        v = codec.limbs_to_ints(np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, self.f))
        assert len(v) == n * self.g and all(x < self.c.q for x in v), "coordinate not canonical"
        v = [x * self.Ri % self.c.q for x in v]
        return [v[i] if self.g == 1 else (v[2 * i], v[2 * i + 1]) for i in range(n)]

    def rand(self, rng):
        return rng.randrange(1, self.c.q) if self.g == 1 else (rng.randrange(1, self.c.q), rng.randrange(self.c.q))

    def jac(self, P, Z, rng=None) -> np.ndarray:
        """(x Z^2, y Z^3, Z); P None: Z = 0 beside garbage X, Y (rng) or ark's (0, 1, 0)."""
        Fo = self.Fo
        if P is None:
            return self.limbs(self.rand(rng), self.rand(rng), Fo.zero) if rng else self.limbs(Fo.zero, Fo.one, Fo.zero)
        z2 = Fo.sqr(Z)
        return self.limbs(Fo.mul(P[0], z2), Fo.mul(P[1], Fo.mul(z2, Z)), Z)

    def xyzz(self, P, z, rng) -> np.ndarray:
        """(x z^2, y z^3, z^2, z^3); P None: zz = 0 beside garbage x, y, zzz."""
        Fo = self.Fo
        if P is None:
            return self.limbs(self.rand(rng), self.rand(rng), Fo.zero, self.rand(rng))
        z2 = Fo.sqr(z)
        z3 = Fo.mul(z2, z)
        return self.limbs(Fo.mul(P[0], z2), Fo.mul(P[1], z3), z2, z3)

    def affine_words(self, P) -> np.ndarray:
        """what into_affine / fixed_base_mul / the proof hold for P: (x, y), the identity as the words (0, 0)"""
        return self.limbs(*P) if P is not None else np.zeros(2 * self.f * self.g, dtype=np.uint64)

    def from_jac(self, words):
        X, Y, Z = self.elts(words, 3)
        return self.G.to_affine((X, Y, Z))

    def mul(self, k):
        return self.G.mul(self.G.gen, k % self.c.r) if k % self.c.r else None

    def msum(self, pts):
        acc = None
        for P in pts:
            acc = self.G.add(acc, P)
        return acc


_ENC = {}


def enc(curve, g) -> Enc:
    if (curve, g) not in _ENC:
        _ENC[(curve, g)] = Enc(curve, g)
    return _ENC[(curve, g)]


def edge_scalars(curve):
    """(label, k): the fixed edge set of the issue plus the scalars picked from the CPU run of the split"""
    gl = glv_ref.Glv(curve)
    r, lam = gl.r, gl.lam
    named = [("0", 0), ("1", 1), ("2", 2), ("r-1", r - 1), ("lambda", lam), ("lambda+1", lam + 1), ("r-lambda", r - lam)]
    seen, out = set(), []
    for label, k in named + glv_ref.GLV_EDGE[curve]:
        if k not in seen:
            seen.add(k)
            out.append((label, k))
    return out


# ------------------------------------------------------------------------------------------------------------ fold
@pytest.mark.parametrize("curve,g", CG)
def test_fold(ctx, curve, g):
    E = enc(curve, g)
    c, G = E.c, E.G
    rng = random.Random(101 + g)
    P, Q = E.mul(rng.randrange(c.r)), E.mul(rng.randrange(c.r))
    Z = lambda: E.rand(rng)                                          # noqa: E731
    chain, T = [], P
    for _ in range(64):                                              # 64 different points, cheap: T += Q
        T = G.add(T, Q)
        chain.append(T)
    cases = [("k = 0", []), ("k = 1", [P]), ("[P, P]", [P, P]), ("[P, -P]", [P, G.neg(P)]), ("[P, -P, Q]", [P, G.neg(P), Q]),
             ("identity first", [None, P, Q]), ("identity in the middle", [P, None, Q]), ("identity last", [P, Q, None]),
             ("identities only", [None, None, None]), ("[inf, P, inf, P, inf]", [None, P, None, P, None]),
             ("[P, P, P, -P, Q, -Q]", [P, P, P, G.neg(P), Q, G.neg(Q)]), ("64 points", chain)]
    asserted = 0
    for name, pts in cases:
        # identities: Z = 0 beside garbage X, Y; the same point twice: under two different Z
        words = [E.jac(T, Z(), rng) for T in pts]
        xyz = np.concatenate(words) if words else np.zeros(0, dtype=np.uint64)
        got = E.from_jac(ctx.fold(c, g, xyz))
        assert got == E.msum(pts), (curve, g, name)
        asserted += 1
    # Z = 1 and Z = p - 1 on both sides of a doubling, and ark's (0, 1, 0) as the identity
    one, m1 = E.Fo.one, E.Fo.neg(E.Fo.one)
    for name, words, want in (("[P (Z = 1), P (Z = -1)]", [E.jac(P, one), E.jac(P, m1)], G.add(P, P)),
                              ("[(0, 1, 0), P]", [E.jac(None, None), E.jac(P, one)], P),
                              ("[(0, 1, 0)]", [E.jac(None, None)], None)):
        assert E.from_jac(ctx.fold(c, g, np.concatenate(words))) == want, (curve, g, name)
        asserted += 1
    print(f"fold {curve} G{g}: generated {len(cases) + 3}, asserted {asserted}")
    assert asserted == len(cases) + 3


# ------------------------------------------------------------------------------------------------------------ into_affine
@pytest.mark.parametrize("curve,g", CG)
def test_into_affine(ctx, curve, g):
    E = enc(curve, g)
    c, Fo = E.c, E.Fo
    rng = random.Random(202 + g)
    pts = [E.G.gen] + [E.mul(rng.randrange(c.r)) for _ in range(3)]
    m1 = Fo.neg(Fo.one)
    zs = [("Z = 1", Fo.one), ("Z = p-1", m1), ("Z = 2", Fo.small(Fo.one, 2))] + [("random Z", E.rand(rng)) for _ in range(4)]
    if g == 2:
        zs += [("Z = u", (0, 1)), ("Z = (p-1)(1 + u)", (c.q - 1, c.q - 1))]
    cases = [(name, P, E.jac(P, Z)) for P in pts for name, Z in zs]
    cases += [("Z = 0, garbage X, Y", None, E.jac(None, None, rng)) for _ in range(3)] + [("(0, 1, 0)", None, E.jac(None, None))]
    cases += [("Z = 0, X = Y = 0", None, E.limbs(Fo.zero, Fo.zero, Fo.zero))]
    asserted = 0
    for name, P, words in cases:
        xy, inf = ctx.into_affine(c, g, words)
        assert inf == (P is None), (curve, g, name, inf)
        assert np.array_equal(xy, E.affine_words(P)), (curve, g, name)             # the identity: flag 1, words (0, 0)
        asserted += 1
    print(f"into_affine {curve} G{g}: generated {len(cases)}, asserted {asserted}")
    assert asserted == len(cases)


# ------------------------------------------------------------------------------------------------------------ fixed_base_mul
@pytest.mark.parametrize("curve,g", CG)
def test_fixed_base_mul(ctx, curve, g):
    """zkp_accel.h: "scalars canonical", so [r, 2^(BITS+1)) is outside the contract: r, r+1, r+2 are NOT passed, and of 2^e, 2^e - 1
    (e up to the top bit fixed_base_kernel reads: 254 on BN254, 255 on BLS12-381) those below r.  2^e P comes from e doublings and
    (2^e - 1) P = 2^e P - P by the affine group law, everything else from oracle/pyref's scalar multiplication."""
    E = enc(curve, g)
    c, G = E.c, E.G
    r = c.r
    top = {"bn254": 254, "bls12_381": 255}[curve]
    rng = random.Random(303 + g)
    scal = [0, 1, 2, 3, r - 1, r - 2, (r + 1) // 2, (r - 1) // 2] + [k for _, k in edge_scalars(curve)]
    pw = [e for e in range(top + 1) if (1 << e) < r]
    assert pw[-1] == r.bit_length() - 1
    asserted = generated = 0
    for bname, B in (("generator", G.gen), ("random point", E.mul(rng.randrange(1, r)))):
        want = [G.mul(B, k) if k else None for k in scal]
        D = B
        ks = list(scal)
        for e in pw:                                                 # D = 2^e B
            ks += [1 << e, (1 << e) - 1]
            want += [D, G.add(D, G.neg(B))]
            D = G.add(D, D)
        generated += len(ks)
        xy, inf = ctx.fixed_base_mul(c, g, E.limbs(*B), codec.ints_to_limbs(ks, 4))
        for k, P, row, fl in zip(ks, want, xy, inf):
            assert int(fl) == int(P is None), (curve, g, bname, hex(k))
            assert np.array_equal(row, E.affine_words(P)), (curve, g, bname, hex(k))
            asserted += 1
    print(f"fixed_base_mul {curve} G{g}: generated {generated}, asserted {asserted}")
    assert asserted == generated


# ------------------------------------------------------------------------------------------------------------ assembly
def proof_points(curve, out, inf):
    """(a, b, c) of the proof words A | B | C; a flagged identity must come with the words (0, 0)"""
    E1, E2 = enc(curve, 1), enc(curve, 2)
    f = E1.f
    parts = [(E1, out[:2 * f]), (E2, out[2 * f:6 * f]), (E1, out[6 * f:8 * f])]
    res = []
    for (E, w), fl in zip(parts, inf):
        assert fl in (0, 1)
        if fl:
            assert not np.asarray(w).any(), "identity flag beside non-zero words"
            res.append(None)
        else:
            x, y = E.elts(w, 2)
            assert E.G.on_curve((x, y))
            res.append((x, y))
    return res


def expected_proof(curve, logs, r_, s_):
    a, b1, b2, h, l = logs
    E1, E2 = enc(curve, 1), enc(curve, 2)
    return [E1.mul(a), E2.mul(b2), E1.mul(s_ * a + r_ * b1 + h + l)]


def exceptional_logs(curve, r_, s_, rng):
    """(name, (a, b1, b2, h, l)) for r_, s_ != 0"""
    n = get_curve(curve).r
    a, b1, b2, h, l = [rng.randrange(1, n) for _ in range(5)]
    ri = pow(r_, -1, n)
    t = (s_ * a + r_ * b1) % n
    return [("generic", (a, b1, b2, h, l)),
            ("a = 0", (0, b1, b2, h, l)),
            ("b1 = 0", (a, 0, b2, h, l)),
            ("a = b1 = 0", (0, 0, b2, h, l)),
            ("s a == r b1", (a, s_ * a * ri % n, b2, h, l)),                     # part 1's last addition doubles
            ("s a == -r b1", (a, -s_ * a * ri % n, b2, h, l)),                   # T is the identity
            ("h + l == -(s a + r b1)", (a, b1, b2, h, (-t - h) % n)),            # proof.c is the identity
            ("h == -(s a + r b1), l = 0", (a, b1, b2, -t % n, 0)),
            ("T + h == l", (a, b1, b2, h, (t + h) % n)),                         # part 2's second addition doubles
            ("h = 0", (a, b1, b2, 0, l)),
            ("l = 0", (a, b1, b2, h, 0)),
            ("h = l = 0", (a, b1, b2, 0, 0)),
            ("b2 = 0", (a, b1, 0, h, l)),
            ("everything 0", (0, 0, 0, 0, 0))]


def jac_sums(curve, logs, rng):
    """A | B1 | B2 | H | L as Jacobian words, each under a random Z; a zero log: Z = 0 beside garbage"""
    E1, E2 = enc(curve, 1), enc(curve, 2)
    return np.concatenate([E.jac(E.mul(k), E.rand(rng), rng) for E, k in zip((E1, E1, E2, E1, E1), logs)])


@pytest.mark.parametrize("curve", CURVES)
def test_assemble_scalar_edges(ctx, curve):
    """r x s over EDGE x EDGE (every pair has both from the set) on fixed generic sums"""
    c = get_curve(curve)
    rng = random.Random(404)
    logs = tuple(rng.randrange(1, c.r) for _ in range(5))
    sums = jac_sums(curve, logs, rng)
    edge = edge_scalars(curve)
    E1 = enc(curve, 1)
    a, b1, b2, h, l = logs
    A, B = E1.mul(a), enc(curve, 2).mul(b2)
    asserted, t0 = 0, time.perf_counter()
    for rl, r_ in edge:
        for sl, s_ in edge:
            out, inf = groth16.assemble(ctx, c, sums, r_, s_)
            got = proof_points(curve, out, inf)
            assert got == [A, B, E1.mul(s_ * a + r_ * b1 + h + l)], (curve, "r = " + rl, "s = " + sl)
            asserted += 1
    print(f"assemble {curve}: generated {len(edge) ** 2}, asserted {asserted}, {time.perf_counter() - t0:.2f} s")
    assert asserted == len(edge) ** 2


def fixed_pairs(curve):
    """(r, s) pairs of the exceptional-sum tests, both from EDGE and non-zero; the first one has k2 < 0 in both chains"""
    e = dict(edge_scalars(curve))
    return [(e["signs (+, -)"], e["max |k2|"]), (e["lambda"], e["r-1"]), (2, e["r-lambda"])]


@pytest.mark.parametrize("curve", CURVES)
def test_assemble_exceptional_sums(ctx, curve):
    c = get_curve(curve)
    rng = random.Random(505)
    asserted = generated = 0
    for r_, s_ in fixed_pairs(curve):
        for name, logs in exceptional_logs(curve, r_, s_, rng):
            generated += 1
            out, inf = groth16.assemble(ctx, c, jac_sums(curve, logs, rng), r_, s_)
            want = expected_proof(curve, logs, r_, s_)
            assert list(inf) == [int(P is None) for P in want], (curve, name, hex(r_), hex(s_), list(inf))
            assert proof_points(curve, out, inf) == want, (curve, name, hex(r_), hex(s_))
            asserted += 1
    print(f"assemble exceptional {curve}: generated {generated}, asserted {asserted}")
    assert asserted == generated


def spread(v, world, mode, n, rng):
    """`world` rank contributions with sum v (mod n): random, the identity on rank 1 only, or two ranks that cancel"""
    if world == 1:
        return [v]
    if mode == 1:
        x = rng.randrange(1, n)
        return [x, 0] + [0] * (world - 3) + [(v - x) % n]
    if mode == 2:
        x = rng.randrange(1, n)
        return [x, (-x) % n] + [0] * (world - 3) + [v]
    xs = [rng.randrange(1, n) for _ in range(world - 1)]
    return xs + [(v - sum(xs)) % n]


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("curve", CURVES)
def test_fold_assemble_dev(ctx, curve, world):
    """The same exceptional slot contents as XYZZ in a device buffer of world x partials_bytes (5 slots of one G2 XYZZ point's size,
    a G1 point at the front of its slot).  World 3: every slot is spread over the ranks at random, with the identity on one rank
    only, or with two ranks that cancel — in turn, so that each slot meets each."""
    c = get_curve(curve)
    E1, E2 = enc(curve, 1), enc(curve, 2)
    rng = random.Random(606 + world)
    pb = groth16.partials_bytes(ctx, c)
    slot = pb // 5 // 8                                              # uint64 words
    assert pb == 5 * 8 * slot and slot == 8 * c.fq_limbs == E2.xyzz(E2.G.gen, E2.Fo.one, rng).size
    r_, s_ = fixed_pairs(curve)[0]
    asserted = generated = 0
    for i, (name, logs) in enumerate(exceptional_logs(curve, r_, s_, rng)):
        generated += 1
        buf = np.frombuffer(rng.randbytes(world * pb), dtype=np.uint64).copy().reshape(world, 5, slot)      # padding: garbage
        for j, (E, v) in enumerate(zip((E1, E1, E2, E1, E1), logs)):
            for rank, part in enumerate(spread(v, world, (i + j) % 3, c.r, rng)):
                w = E.xyzz(E.mul(part), E.rand(rng), rng)
                buf[rank, j, :w.size] = w
        d = ctx.to_device(buf)
        try:
            out, inf = groth16.fold_assemble_dev(ctx, c, d, world, r_, s_)
        finally:
            ctx.dev_free(d)
        want = expected_proof(curve, logs, r_, s_)
        assert list(inf) == [int(P is None) for P in want], (curve, world, name, list(inf))
        assert proof_points(curve, out, inf) == want, (curve, world, name)
        asserted += 1
    print(f"fold_assemble_dev {curve} world {world}: generated {generated}, asserted {asserted}")
    assert asserted == generated
