"""Python-integer restatement of asvc/src/lib.rs, function by function: key_gen (:76-158), commit (:160-180), prove_pos (:182-225),
verify_pos (:227-285), verify_upk (:287-337), update_commit (:339-363), update_proof (:365-403), aggregate_proofs (:405-439).

The reference cannot be built here (no cargo), so parity with it stays UNPINNED BY THE REFERENCE: what is pinned is this restatement,
whose verifiers accept what its provers produce and reject tampered inputs (tests/test_asvc_ref.py), over the ark contracts that
oracle/pyref restates (Domain, Group, Pairing; see oracle/README.md).  The division of prove_pos is plain long division, not the
partial-fraction identity the device kernel rests on; `quotient_by_identity` states that identity separately so that a test can
compare the two.

Scalars are canonical integers, G1 points (x, y) or None, G2 points ((x0, x1), (y0, y1)) or None, as in oracle/pyref."""
from __future__ import annotations

from dataclasses import dataclass, field

from oracle.pyref.curves import Group
from oracle.pyref.fields import CURVES
from oracle.pyref.ntt import Domain
from oracle.pyref.pairing import Pairing


def curve_of(curve):
    return CURVES[curve] if not hasattr(curve, "two_adicity") else curve


def domain_of(curve, n: int) -> Domain:
    return Domain(curve_of(curve), n)


# ---------------------------------------------------------------- dense polynomials over Fr, low coefficient first
def poly_mul(a, b, r):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % r
    return out


def poly_divmod(num, den, r):
    """long division (DenseOrSparsePolynomial::divide_with_q_and_r): (q, rem) with len(q) = len(num) - len(den) + 1 (or [] if
    shorter); trailing zero coefficients are kept, so positions line up with the device's n - k outputs"""
    den = list(den)
    while den and den[-1] == 0:
        den.pop()
    assert den, "division by the zero polynomial"
    rem, dn = [x % r for x in num], len(den) - 1
    if len(rem) <= dn:
        return [], rem
    lead_inv = pow(den[-1], -1, r)
    q = [0] * (len(rem) - dn)
    for t in range(len(q) - 1, -1, -1):
        c = rem[t + dn] * lead_inv % r
        q[t] = c
        if c:
            for j, d in enumerate(den):
                rem[t + j] = (rem[t + j] - c * d) % r
    return q, rem[:dn]


def poly_eval(p, x, r):
    acc = 0
    for c in reversed(p):
        acc = (acc * x + c) % r
    return acc


def vanishing(points, omega, r):
    """A_I(X) = prod (X - omega^p)"""
    a = [1]
    for p in points:
        a = poly_mul(a, [(-pow(omega, p, r)) % r, 1], r)
    return a


def subset_weights(curve, n: int, points):
    """c_i = 1 / A_I'(omega^p_i) as aggregate_proofs forms it (:425-431): A_I / (X - omega_i) evaluated at omega_i, inverted"""
    d = domain_of(curve, n)
    r, w = d.r, d.group_gen
    a = vanishing(points, w, r)
    out = []
    for p in points:
        wi = pow(w, p, r)
        quo, rem = poly_divmod(a, [(-wi) % r, 1], r)
        assert not any(rem)
        out.append(pow(poly_eval(quo, wi, r), -1, r))
    return out


def subset_weights_direct(curve, n: int, points):
    """the same weights as 1 / prod_{j != i} (omega_i - omega_j): O(k^2), for large subsets"""
    d = domain_of(curve, n)
    r = d.r
    ws = [pow(d.group_gen, p, r) for p in points]
    out = []
    for i, wi in enumerate(ws):
        acc = 1
        for j, wj in enumerate(ws):
            if j != i:
                acc = acc * (wi - wj) % r
        out.append(pow(acc, -1, r))
    return out


def quotient(curve, phi, points):
    """floor(Phi / A_I) by long division: n - k coefficients for n = len(phi) (a power of two)"""
    d = domain_of(curve, len(phi))
    assert d.size == len(phi)
    return poly_divmod(phi, vanishing(points, d.group_gen, d.r), d.r)[0]


def quotient_by_identity(curve, phi, points):
    """q[t] = sum_i c_i S_i[t], S_i[t] = Phi[t+1] + omega_i S_i[t+1], S_i[n-1] = 0; returns all n - 1 values (the top k - 1 are zero)"""
    n = len(phi)
    d = domain_of(curve, n)
    r = d.r
    cs = subset_weights(curve, n, points)
    q = [0] * (n - 1)
    for c, p in zip(cs, points):
        wi, s = pow(d.group_gen, p, r), 0
        for t in range(n - 2, -1, -1):
            s = (phi[t + 1] + wi * s) % r
            q[t] = (q[t] + c * s) % r
    return q


# ---------------------------------------------------------------- the scheme
@dataclass
class UpdateKey:
    ai: tuple
    ui: tuple


@dataclass
class ProvingKey:
    powers_of_g1: list
    l_of_g1: list
    update_keys: list


@dataclass
class VerificationKey:
    powers_of_g1: list
    powers_of_g2: list
    a: tuple


@dataclass
class Parameters:
    proving_key: ProvingKey
    verification_key: VerificationKey
    scalars: dict = field(default_factory=dict)        # the exponents (tests only): "a", "l", "u" lists and "a_tau"


def key_scalars(curve, n: int, tau: int):
    """the exponents of key_gen: (size, powers of tau (size + 1), A(tau), a_i, l_i, u_i)"""
    d = domain_of(curve, n)
    r, size, w = d.r, d.size, d.group_gen
    a_tau = (pow(tau, size, r) - 1) % r
    a_s, l_s, u_s = [], [], []
    for i in range(size):
        wi = pow(w, i, r)
        div = pow((tau - wi) % r, -1, r)                  # ValueError when tau lies in the domain
        ai = a_tau * div % r
        li = ai * wi % r * d.size_inv % r
        a_s.append(ai)
        l_s.append(li)
        u_s.append((li - 1) * div % r)
    return size, [pow(tau, j, r) for j in range(size + 1)], a_tau, a_s, l_s, u_s


def key_gen(curve, n: int, tau: int, g1, g2) -> Parameters:
    c = curve_of(curve)
    G1, G2 = Group(c, 1), Group(c, 2)
    size, powers, a_tau, a_s, l_s, u_s = key_scalars(c, n, tau)
    p1 = [G1.mul(g1, s) for s in powers]
    p2 = [G2.mul(g2, s) for s in powers]
    upks = [UpdateKey(G1.mul(g1, a), G1.mul(g1, u)) for a, u in zip(a_s, u_s)]
    pk = ProvingKey(p1, [G1.mul(g1, s) for s in l_s], upks)
    vk = VerificationKey(p1, p2, G1.mul(g1, a_tau))
    return Parameters(pk, vk, {"a_tau": a_tau, "a": a_s, "l": l_s, "u": u_s, "powers": powers})


def commit(curve, pk: ProvingKey, values):
    assert 1 <= len(values) <= len(pk.l_of_g1)
    return Group(curve_of(curve), 1).msm_naive(pk.l_of_g1, values)


def witness_polynomial(curve, n: int, values, points):
    """the quotient of prove_pos: values padded to the domain, inverse transform, long division"""
    d = domain_of(curve, n)
    phi = d.ifft(list(values) + [0] * (d.size - len(values)))
    return poly_divmod(phi, vanishing(points, d.group_gen, d.r), d.r)[0]


def prove_pos(curve, pk: ProvingKey, values, points):
    q = witness_polynomial(curve, len(pk.powers_of_g1) - 1, values, points)
    return Group(curve_of(curve), 1).msm_naive(pk.powers_of_g1, q)


def prove_pos_in_exponent(curve, n: int, tau: int, g1, values, points):
    """[q(tau)] g1: the same proof without a Python MSM (for sizes where one would take minutes)"""
    c = curve_of(curve)
    return Group(c, 1).mul(g1, poly_eval(witness_polynomial(c, n, values, points), tau, c.r))


def verify_pos(curve, vk: VerificationKey, commitment, point_values, points, proof, omega) -> bool:
    c = curve_of(curve)
    r = c.r
    G1, G2 = Group(c, 1), Group(c, 2)
    a_poly = vanishing(points, omega, r)
    r_poly = [0]
    for p, v in zip(points, point_values):
        wi = pow(omega, p, r)
        l_poly, _ = poly_divmod(a_poly, [(-wi) % r, 1], r)
        scale = v * pow(poly_eval(l_poly, wi, r), -1, r) % r
        l_poly = [x * scale % r for x in l_poly]
        r_poly = [(x + y) % r for x, y in zip(r_poly + [0] * (len(l_poly) - len(r_poly)), l_poly + [0] * (len(r_poly) - len(l_poly)))]
    r_value = G1.msm_naive(vk.powers_of_g1, r_poly)
    inner = G1.add(commitment, G1.neg(r_value))
    a_value = G2.msm_naive(vk.powers_of_g2, a_poly)
    # e(inner, g2) == e(w, a_value)
    return Pairing(c).product_is_one([(inner, vk.powers_of_g2[0]), (G1.neg(proof), a_value)])


def verify_upk(curve, vk: VerificationKey, point: int, upk: UpdateKey, omega) -> bool:
    c = curve_of(curve)
    r = c.r
    G1, G2 = Group(c, 1), Group(c, 2)
    n = len(vk.powers_of_g1) - 1
    wi = pow(omega, point, r)
    inner = G2.add(vk.powers_of_g2[1], G2.neg(G2.mul(vk.powers_of_g2[0], wi)))
    pr = Pairing(c)
    rs1 = pr.product_is_one([(upk.ai, inner), (G1.neg(vk.a), vk.powers_of_g2[0])])
    l_value = G1.mul(upk.ai, wi * pow(n, -1, r) % r)
    inner2 = G1.add(l_value, G1.neg(vk.powers_of_g1[0]))
    rs2 = pr.product_is_one([(inner2, vk.powers_of_g2[0]), (G1.neg(upk.ui), inner)])
    return rs1 and rs2


def update_commit(curve, commitment, delta: int, point: int, upk: UpdateKey, omega, n: int):
    c = curve_of(curve)
    G1 = Group(c, 1)
    l_value = G1.mul(upk.ai, pow(omega, point, c.r) * pow(n, -1, c.r) % c.r)
    return G1.add(commitment, G1.mul(l_value, delta))


def update_proof(curve, proof, delta: int, point_i: int, point_j: int, upk_i: UpdateKey, upk_j: UpdateKey, omega, n: int):
    c = curve_of(curve)
    r = c.r
    G1 = Group(c, 1)
    if point_i == point_j:
        return G1.add(proof, G1.mul(upk_i.ui, delta))
    wi, wj = pow(omega, point_i, r), pow(omega, point_j, r)
    c1, c2 = pow((wj - wi) % r, -1, r), pow((wi - wj) % r, -1, r)
    w_ij = G1.add(G1.mul(upk_j.ai, c1), G1.mul(upk_i.ai, c2))
    u_ij = G1.mul(w_ij, wj * pow(n, -1, r) % r)
    return G1.add(proof, G1.mul(u_ij, delta))


def aggregate_proofs(curve, n: int, points, proofs):
    c = curve_of(curve)
    G1 = Group(c, 1)
    acc = None
    for cw, pf in zip(subset_weights(c, n, points), proofs):
        acc = G1.add(acc, G1.mul(pf, cw))
    return acc
