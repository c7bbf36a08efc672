"""CPU: tests/sumcheck_ref.py against closed forms, a hand-computed example and the identities a sum-check transcript must obey,
so that the reference the device tests compare with is pinned without a GPU."""
import hashlib
import random

import pytest

from tests import sumcheck_ref as ref

R = {"bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "bls12_381": 52435875175126190479447740508185965837690552500527637822603658699938581184513}
CURVES = list(R)


def _sha_challenge(r):
    def ch(coeffs):
        h = hashlib.sha256(b"".join(c.to_bytes(32, "little") for c in coeffs)).digest()
        return int.from_bytes(h, "little") % r
    return ch


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("k", [0, 1, 2, 5])
def test_eval_eq_closed_form_and_unit_vectors(curve, k):
    r = R[curve]
    rng = random.Random(k)
    rx = [rng.randrange(r) for _ in range(k)]
    if k >= 2:
        rx[0], rx[1] = 0, r - 1
    table = ref.eval_eq(rx, r)
    assert len(table) == 1 << k
    for idx in range(1 << k):
        bits = [(idx >> (k - 1 - i)) & 1 for i in range(k)]                    # rx[0] decides the most significant bit
        closed = 1
        for b, x in zip(bits, rx):
            closed = closed * (x if b else 1 - x) % r
        assert table[idx] == closed
        assert table[idx] == ref.eval_eq_x_y(rx, bits, r)                      # = sum_i eq(rx)[i] unit_idx[i]
    assert sum(table) % r == 1


def test_combine_is_lo_plus_x_times_diff():
    r = R["bn254"]
    rng = random.Random(3)
    v = [rng.randrange(r) for _ in range(16)] + [0, r - 1] * 8
    for x in (0, 1, 2, 3, r - 1, rng.randrange(r)):
        assert ref.combine_with_n(v, x, r) == [(v[i] + x * (v[i + 16] - v[i])) % r for i in range(16)]


@pytest.mark.parametrize("kind", [ref.EQ_AB_MINUS_C, ref.PROD2, ref.PROD3])
def test_round_evals_is_combine_with_n(kind):
    r = R["bls12_381"]
    rng = random.Random(kind)
    tables = [[rng.randrange(r) for _ in range(16)] for _ in range(ref.ARITY[kind])]
    tables[0][3], tables[1][11] = 0, r - 1
    g = {ref.EQ_AB_MINUS_C: lambda e, a, b, c: e * (a * b - c), ref.PROD2: lambda a, b: a * b, ref.PROD3: lambda a, b, c: a * b * c}[kind]
    exp = tuple(sum(g(*col) for col in zip(*(ref.combine_with_n(t, x, r) for t in tables))) % r for x in ref.POINTS[kind])
    assert ref.round_evals(kind, tables, r) == exp
    assert exp[0] == sum(g(*col) for col in zip(*(t[:8] for t in tables))) % r


def test_hand_computed_two_variables():
    """eq = [1,2,3,4], a = [1,1,2,3], b = [2,0,1,1], c = [0,1,1,1], claim 11, challenges 2 then 3, worked by hand:
    round 0: g(0..3) = 0, 11, 44, 111 -> 2 X^3 + 5 X^2 + 4 X;  bound at 2: eq = [5,6], a = [3,5], b = [0,2], c = [2,1], claim 44;
    round 1: g(0..3) = -10, 54, 196, 440 -> 4 X^3 + 27 X^2 + 33 X - 10;  bound at 3: eq = 8, a = 9, b = 6, c = -1, claim 440."""
    r = R["bn254"]
    xs = iter([2, 3])
    polys, rx, (va, vb, vc, veq) = ref.phase_one([1, 2, 3, 4], [1, 1, 2, 3], [2, 0, 1, 1], [0, 1, 1, 1], 11, lambda _: next(xs), r)
    assert polys == [[0, 4, 5, 2], [r - 10, 33, 27, 4]]
    assert rx == [2, 3]
    assert (va, vb, vc, veq) == (9, 6, r - 1, 8)
    assert ref.evaluate(polys[1], 3, r) == 440 == veq * (va * vb - vc) % r
    # phase two on the same numbers: abc = [1,2,3,4], z = [2,0,1,1]: g(0) = 2, g(1) = 7, g(2) = 6*0 + 6*2 = 12 -> claim 9
    xs = iter([2, 3])
    polys, ry, (vs, vz) = ref.phase_two([1, 2, 3, 4], [2, 0, 1, 1], 9, lambda _: next(xs), r)
    assert polys[0] == [2, 5, 0]                                               # 0 X^2 + 5 X + 2
    assert polys[1] == [0, 10, 2]                                              # bound at 2: [5,6], [0,2]: g = 0, 12, 28
    assert (vs, vz) == (8, 6)                                                  # bound at 3: 5 + 3, 0 + 6
    assert ref.evaluate(polys[1], 3, r) == 48


def _instance(r, k, seed, satisfied=True):
    rng = random.Random(seed)
    n = 1 << k
    a = [rng.randrange(r) for _ in range(n)]
    b = [rng.randrange(r) for _ in range(n)]
    c = [x * y % r for x, y in zip(a, b)]
    if not satisfied:
        c[n // 3] = (c[n // 3] + 1) % r
    tau = [rng.randrange(r) for _ in range(k)]
    return ref.eval_eq(tau, r), a, b, c


@pytest.mark.parametrize("curve", CURVES)
def test_phase_one_round_identities(curve):
    r = R[curve]
    k = 6
    eq, a, b, c = _instance(r, k, 11)
    ch = _sha_challenge(r)
    polys, rx, (va, vb, vc, veq) = ref.phase_one(eq, a, b, c, 0, ch, r)
    claim = 0
    for i, poly in enumerate(polys):
        # g(1) directly from the tables bound by rx[:i]
        te, ta, tb, tc = eq, a, b, c
        for x in rx[:i]:
            te, ta, tb, tc = (ref.combine_with_r(t, x, r) for t in (te, ta, tb, tc))
        h = len(te) // 2
        g0 = sum(te[j] * (ta[j] * tb[j] - tc[j]) for j in range(h)) % r
        g1 = sum(te[j] * (ta[j] * tb[j] - tc[j]) for j in range(h, 2 * h)) % r
        assert (g0 + g1) % r == claim
        assert ref.evaluate(poly, 0, r) == g0 and ref.evaluate(poly, 1, r) == g1
        assert rx[i] == ch(poly)
        claim = ref.evaluate(poly, rx[i], r)
    assert claim == veq * (va * vb - vc) % r
    eq_rx = ref.eval_eq(rx, r)
    assert va == sum(x * y for x, y in zip(a, eq_rx)) % r
    assert vb == sum(x * y for x, y in zip(b, eq_rx)) % r


def test_unsatisfied_instance_breaks_the_round_identity():
    r = R["bn254"]
    eq, a, b, c = _instance(r, 5, 12, satisfied=False)
    h = len(eq) // 2
    g0 = sum(eq[j] * (a[j] * b[j] - c[j]) for j in range(h)) % r
    g1 = sum(eq[j] * (a[j] * b[j] - c[j]) for j in range(h, 2 * h)) % r
    assert (g0 + g1) % r != 0                                                  # the claim 0 of a satisfied instance
    polys, rx, (va, vb, vc, veq) = ref.phase_one(eq, a, b, c, 0, _sha_challenge(r), r)
    assert ref.evaluate(polys[-1], rx[-1], r) != veq * (va * vb - vc) % r


@pytest.mark.parametrize("curve", CURVES)
def test_phase_two_and_cubic_final_claims(curve):
    r = R[curve]
    rng = random.Random(21)
    n = 32
    rnd = lambda: [rng.randrange(r) for _ in range(n)]                        # noqa: E731
    abc, z = rnd(), rnd()
    claim = sum(x * y for x, y in zip(abc, z)) % r
    polys, ry, (vs, vz) = ref.phase_two(abc, z, claim, _sha_challenge(r), r)
    assert ref.evaluate(polys[-1], ry[-1], r) == vs * vz % r
    assert vz == sum(x * y for x, y in zip(z, ref.eval_eq(ry, r))) % r
    a_par, b_par, c_par = [rnd() for _ in range(3)], [rnd() for _ in range(3)], rnd()
    a_seq, b_seq, c_seq = [rnd() for _ in range(2)], [rnd() for _ in range(2)], [rnd() for _ in range(2)]
    coeffs = [rng.randrange(r) for _ in range(5)]
    terms = [(a, b, c_par) for a, b in zip(a_par, b_par)] + list(zip(a_seq, b_seq, c_seq))
    claim = sum(w * sum(x * y * v for x, y, v in zip(*t)) for w, t in zip(coeffs, terms)) % r
    polys, rs, (fa, fb, fc), (sa, sb, sc) = ref.cubic_batched(a_par, b_par, c_par, a_seq, b_seq, c_seq, coeffs, claim,
                                                               _sha_challenge(r), r)
    fin = [x * y * fc for x, y in zip(fa, fb)] + [x * y * v for x, y, v in zip(sa, sb, sc)]
    assert ref.evaluate(polys[-1], rs[-1], r) == sum(w * f for w, f in zip(coeffs, fin)) % r
    # the spelled-out doublings of :1483-1494 are combine_with_n at 2 and 3
    t2 = [ref.combine_with_n(t, 2, r) for t in terms[0]]
    assert ref._cubic_term(*terms[0], r)[1] == sum(x * y * v for x, y, v in zip(*t2)) % r


def test_r1cs_backbone_satisfied():
    r = R["bn254"]
    rng = random.Random(31)
    rows, nz = 8, 16
    z = [rng.randrange(r) for _ in range(nz)]
    sparse = lambda: [[(rng.randrange(r), rng.randrange(nz)) for _ in range(rng.randrange(1, 4))] for _ in range(rows)]   # noqa: E731
    ma, mb = sparse(), sparse()
    az, bz = ref.matrix_vec(ma, z, r), ref.matrix_vec(mb, z, r)
    # C: one entry per row on a column whose z is non-zero, scaled so that Cz = Az o Bz
    mc = [[(x * y * pow(z[i], -1, r) % r, i)] for i, (x, y) in enumerate(zip(az, bz))]
    tau = [rng.randrange(r) for _ in range(3)]
    abc = lambda va, vb, vc, veq: (va + 1, vb + 2, vc + 3)                    # noqa: E731
    p1, rx, (va, vb, vc, veq), p2, ry, (vs, vz) = ref.r1cs_backbone(ma, mb, mc, z, tau, _sha_challenge(r), abc, _sha_challenge(r), r)
    assert ref.evaluate(p1[-1], rx[-1], r) == veq * (va * vb - vc) % r
    assert veq == ref.eval_eq_x_y(tau, rx, r)
    assert va == sum(x * y for x, y in zip(az, ref.eval_eq(rx, r))) % r
    assert ref.evaluate(p2[-1], ry[-1], r) == vs * vz % r
    assert len(rx) == 3 and len(ry) == 4
