"""Shared reference of the pairing tests (Python integers over oracle/pyref).

Two things live here:

* the expected values: E = Pairing(c).pairing(g1_gen, g2_gen) is computed ONCE per curve per session (the oracle's plain
  square-and-multiply final exponentiation, 0.6 - 1 s) and every other expected GT value follows from it by bilinearity: for
  P = [a] G1 and Q = [b] G2 the device returns E^(s k a b mod r), k = GT_POWER of the curve and s = 1 on BN254, s = r - 1 on
  BLS12-381 (the oracle does not conjugate for the negative x and so returns e^-1 there; see its docstring).  GT has order r, so
  these are 255-bit powers of milliseconds each.
* a model of the device's formulas (csrc/pairing_dev.hpp) in the same tower Fq12 = Fq6[w] / (w^2 - v), Fq6 = Fq2[v] / (v^3 - xi):
  the Karatsuba tower products, the Granger-Scott squaring, the projective Miller loop with inversion-free lines and the two
  hard-part chains.  tests/test_pairing_ref.py holds the model against the oracle, so a wrong formula shows without a device.

An Fq12 is a flat list of six Fq2 pairs over the basis 1, w, ..., w^5 (what oracle.pyref.pairing.Fp12 multiplies); tower
coefficient c_j.c_i (j: power of w, i: power of v) is flat coefficient 2 i + j.
"""
from __future__ import annotations

import functools
import random

from oracle.pyref.curves import Group
from oracle.pyref.fields import CURVES, f2_add, f2_inv, f2_mul, f2_neg, f2_scalar, f2_sqr, f2_sub
from oracle.pyref.pairing import Fp12, Pairing

CURVE_NAMES = ("bn254", "bls12_381")
GT_POWER = {"bn254": 1, "bls12_381": 3}                 # == ckb_zkp_amd.pairing.GT_POWER (test_pairing_ref.py compares)
TOWER_TO_FLAT = [0, 2, 4, 1, 3, 5]                       # ABI position (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) -> power of w


def curve(name):
    return CURVES[name]


@functools.lru_cache(maxsize=None)
def pairing(name) -> Pairing:
    return Pairing(CURVES[name])


@functools.lru_cache(maxsize=None)
def gen_pairing(name):
    """E: the oracle's pairing of the two generators (the one full oracle exponentiation of a session)."""
    pr = pairing(name)
    return tuple(pr.pairing(CURVES[name].g1_gen, CURVES[name].g2_gen))


def sign(name) -> int:
    c = CURVES[name]
    return 1 if name == "bn254" else c.r - 1


def gt_pow(name, e: int):
    """E^e as a flat list."""
    c = CURVES[name]
    return Fp12(c).pow(list(gen_pairing(name)), e % c.r)


def expected_pairing(name, a: int, b: int):
    """What the device returns for e([a] G1, [b] G2)."""
    return expected_product(name, [(a, b)])


def expected_product(name, pairs):
    """What the device returns for prod e([a_i] G1, [b_i] G2): E^(s k sum a_i b_i)."""
    c = CURVES[name]
    e = sum(a * b for a, b in pairs) % c.r
    return gt_pow(name, sign(name) * GT_POWER[name] * e)


@functools.lru_cache(maxsize=None)
def _groups(name):
    return Group(CURVES[name], 1), Group(CURVES[name], 2)


def g1_mul(name, a: int):
    G1, _ = _groups(name)
    return G1.mul(CURVES[name].g1_gen, a % CURVES[name].r)


def g2_mul(name, b: int):
    _, G2 = _groups(name)
    return G2.mul(CURVES[name].g2_gen, b % CURVES[name].r)


def balanced_group(name, size: int, rng: random.Random, off_by_one: bool = False):
    """`size` scalar pairs (a_i, b_i) with sum a_i b_i = 0 mod r (off_by_one: = b_0, one scalar moved by one)."""
    r = CURVES[name].r
    if size == 1:
        pairs = [(0 if not off_by_one else 1, rng.randrange(1, r))]
        return pairs
    pairs = [(rng.randrange(1, r), rng.randrange(1, r)) for _ in range(size - 1)]
    s = sum(a * b for a, b in pairs) % r
    b_last = rng.randrange(1, r)
    pairs.append(((-s) * pow(b_last, -1, r) % r, b_last))
    if off_by_one:
        pairs[0] = ((pairs[0][0] + 1) % r, pairs[0][1])
    return pairs


# ----------------------------------------------------------------------------------------------- the tower, as the device has it
class Tower:
    """Fq12 elements are ((c00, c01, c02), (c10, c11, c12)) of Fq2 pairs."""

    def __init__(self, name):
        c = CURVES[name]
        self.c, self.p, self.xi = c, c.q, c.xi
        self.one2, self.zero2 = (1, 0), (0, 0)
        self.one6 = (self.one2, self.zero2, self.zero2)
        self.zero6 = (self.zero2,) * 3
        self.one = (self.one6, self.zero6)
        self.frob_c = [[self._pow2(c.xi, j * (c.q**k - 1) // 6) for j in range(6)] for k in (1, 2, 3)]

    def _pow2(self, a, e):
        r = (1, 0)
        for bit in bin(e)[2:]:
            r = f2_sqr(r, self.p)
            if bit == "1":
                r = f2_mul(r, a, self.p)
        return r

    # Fq2
    def m2(self, a, b): return f2_mul(a, b, self.p)
    def a2(self, a, b): return f2_add(a, b, self.p)
    def s2(self, a, b): return f2_sub(a, b, self.p)
    def mxi(self, a): return f2_mul(a, self.xi, self.p)

    # Fq6
    def add6(self, a, b): return tuple(self.a2(x, y) for x, y in zip(a, b))
    def sub6(self, a, b): return tuple(self.s2(x, y) for x, y in zip(a, b))
    def neg6(self, a): return tuple(f2_neg(x, self.p) for x in a)
    def mulv6(self, a): return (self.mxi(a[2]), a[0], a[1])

    def mul6(self, a, b):
        m, A, S, xi = self.m2, self.a2, self.s2, self.mxi
        v0, v1, v2 = m(a[0], b[0]), m(a[1], b[1]), m(a[2], b[2])
        c0 = A(v0, xi(S(S(m(A(a[1], a[2]), A(b[1], b[2])), v1), v2)))
        c1 = A(S(S(m(A(a[0], a[1]), A(b[0], b[1])), v0), v1), xi(v2))
        c2 = A(S(S(m(A(a[0], a[2]), A(b[0], b[2])), v0), v2), v1)
        return (c0, c1, c2)

    def mul6_by_01(self, s, c0, c1):
        m, A, S, xi = self.m2, self.a2, self.s2, self.mxi
        aa, bb = m(s[0], c0), m(s[1], c1)
        t1 = A(xi(S(m(A(s[1], s[2]), c1), bb)), aa)
        t3 = A(S(m(A(s[0], s[2]), c0), aa), bb)
        t2 = S(S(m(A(c0, c1), A(s[0], s[1])), aa), bb)
        return (t1, t2, t3)

    def inv6(self, a):
        m, A, S, xi = self.m2, self.a2, self.s2, self.mxi
        t0 = S(m(a[0], a[0]), xi(m(a[1], a[2])))
        t1 = S(xi(m(a[2], a[2])), m(a[0], a[1]))
        t2 = S(m(a[1], a[1]), m(a[0], a[2]))
        d = A(m(a[0], t0), xi(A(m(a[2], t1), m(a[1], t2))))
        di = f2_inv(d, self.p)
        return (m(t0, di), m(t1, di), m(t2, di))

    # Fq12
    def mul(self, a, b):
        v0, v1 = self.mul6(a[0], b[0]), self.mul6(a[1], b[1])
        c1 = self.sub6(self.sub6(self.mul6(self.add6(a[0], a[1]), self.add6(b[0], b[1])), v0), v1)
        return (self.add6(v0, self.mulv6(v1)), c1)

    def sqr(self, a):
        ab = self.mul6(a[0], a[1])
        c0 = self.mul6(self.add6(a[0], a[1]), self.add6(a[0], self.mulv6(a[1])))
        c0 = self.sub6(self.sub6(c0, ab), self.mulv6(ab))
        return (c0, self.add6(ab, ab))

    def conj(self, a): return (a[0], self.neg6(a[1]))

    def inv(self, a):
        t = self.sub6(self.mul6(a[0], a[0]), self.mulv6(self.mul6(a[1], a[1])))
        t = self.inv6(t)
        return (self.mul6(a[0], t), self.neg6(self.mul6(a[1], t)))

    def frob(self, a, k):
        out = [[None] * 3, [None] * 3]
        for j in range(2):
            for i in range(3):
                x = a[j][i]
                if k & 1:
                    x = (x[0], (-x[1]) % self.p)
                out[j][i] = self.m2(x, self.frob_c[k - 1][2 * i + j])
        return (tuple(out[0]), tuple(out[1]))

    def mul_by_line(self, f, a0, a1, b0, b1):
        """f (A + B w), A = a0 + a1 v, B = b0 + b1 v: three Fq6 products by (c0, c1, 0)."""
        v0 = self.mul6_by_01(f[0], a0, a1)
        v1 = self.mul6_by_01(f[1], b0, b1)
        c1 = self.mul6_by_01(self.add6(f[0], f[1]), self.a2(a0, b0), self.a2(a1, b1))
        c1 = self.sub6(self.sub6(c1, v0), v1)
        return (self.add6(v0, self.mulv6(v1)), c1)

    def cyclotomic_sqr(self, a):
        """Granger-Scott: three Fq4 squarings, for elements of the cyclotomic subgroup only."""
        m, A, S, xi = self.m2, self.a2, self.s2, self.mxi

        def fp4_sqr(x, y):
            t = m(x, y)
            return S(S(m(A(x, y), A(xi(y), x)), t), xi(t)), A(t, t)

        z0, z4, z3 = a[0]
        z2, z1, z5 = a[1]
        t0, t1 = fp4_sqr(z0, z1)
        t2, t3 = fp4_sqr(z2, z3)
        t4, t5 = fp4_sqr(z4, z5)

        def minus(t, z):                                    # 3 t - 2 z
            d = S(t, z)
            return A(A(d, d), t)

        def plus(t, z):                                     # 3 t + 2 z
            d = A(t, z)
            return A(A(d, d), t)

        z0, z1 = minus(t0, z0), plus(t1, z1)
        z2 = plus(xi(t5), z2)
        z3, z4, z5 = minus(t4, z3), minus(t2, z4), plus(t3, z5)
        return ((z0, z4, z3), (z2, z1, z5))

    def cyc_pow_abs_x(self, a):
        r = a
        for bit in bin(self.c.x_param)[3:]:
            r = self.cyclotomic_sqr(r)
            if bit == "1":
                r = self.mul(r, a)
        return r

    def pow_x(self, a):
        """a^x for a in the cyclotomic subgroup (x negative on BLS12-381)."""
        r = self.cyc_pow_abs_x(a)
        return r if self.c.name == "bn254" else self.conj(r)

    def final_exp(self, f):
        """f^(GT_POWER (q^12 - 1) / r), by the device's chain."""
        mul, sq, conj = self.mul, self.cyclotomic_sqr, self.conj
        f = mul(conj(f), self.inv(f))
        f = mul(self.frob(f, 2), f)
        if self.c.name == "bn254":
            a = self.pow_x(f)
            b = self.pow_x(a)
            c = self.pow_x(b)
            b6 = sq(mul(sq(b), b))
            b12 = sq(b6)
            b18 = mul(b12, b6)
            b30 = mul(b18, b12)
            a6 = sq(mul(sq(a), a))
            a12 = sq(a6)
            a18 = mul(a12, a6)
            c8 = sq(sq(sq(c)))
            c36 = sq(sq(mul(c8, c)))
            y3 = self.frob(f, 3)
            y2 = self.frob(mul(b6, f), 2)
            y1 = self.frob(mul(conj(mul(mul(c36, b18), a12)), f), 1)
            y0 = conj(mul(mul(mul(c36, b30), a18), sq(f)))
            return mul(mul(y3, y2), mul(y1, y0))
        y = mul(self.pow_x(f), conj(f))                     # f^(x - 1)
        y = mul(self.pow_x(y), conj(y))                     # f^((x - 1)^2)
        t1 = mul(self.pow_x(y), self.frob(y, 1))            # ^(x + q)
        t2 = mul(mul(self.pow_x(self.pow_x(t1)), self.frob(t1, 2)), conj(t1))   # ^(x^2 + q^2 - 1)
        return mul(t2, mul(sq(f), f))

    # the Miller loop on homogeneous projective coordinates of the twist, lines without inversions
    def miller(self, P, Q):
        if P is None or Q is None:
            return self.one
        c, p = self.c, self.p
        m, A, S = self.m2, self.a2, self.s2
        sc = lambda a, k: f2_scalar(a, k, p)
        xP, yP = P
        two_inv = pow(2, -1, p)
        bt = c.g2_b

        def ell(f, c0, c1, c2):
            if c.twist_is_d:
                return self.mul_by_line(f, sc(c0, yP), self.zero2, sc(c1, xP), c2)
            return self.mul_by_line(f, c0, sc(c1, xP), self.zero2, sc(c2, yP))

        def dbl(T):
            X, Y, Z = T
            a = sc(m(X, Y), two_inv)
            b, cc = m(Y, Y), m(Z, Z)
            e = m(bt, A(A(cc, cc), cc))
            f3 = A(A(e, e), e)
            g = sc(A(b, f3), two_inv)
            h = S(m(A(Y, Z), A(Y, Z)), A(b, cc))
            i = S(e, b)
            j = m(X, X)
            e2 = m(e, e)
            T = (m(a, S(b, f3)), S(m(g, g), A(A(e2, e2), e2)), m(b, h))
            j3 = A(A(j, j), j)
            nh = f2_neg(h, p)
            return T, ((nh, j3, i) if c.twist_is_d else (i, j3, nh))

        def add(T, q):
            X, Y, Z = T
            theta = S(Y, m(q[1], Z))
            lam = S(X, m(q[0], Z))
            cc, d = m(theta, theta), m(lam, lam)
            e = m(lam, d)
            f = m(Z, cc)
            g = m(X, d)
            h = S(A(e, f), A(g, g))
            T = (m(lam, h), S(m(theta, S(g, h)), m(e, Y)), m(Z, e))
            j = S(m(theta, q[0]), m(lam, q[1]))
            nt = f2_neg(theta, p)
            return T, ((lam, nt, j) if c.twist_is_d else (j, nt, lam))

        loop = 6 * c.x_param + 2 if c.name == "bn254" else c.x_param
        f, T = self.one, (Q[0], Q[1], self.one2)
        for bit in bin(loop)[3:]:
            T, l = dbl(T)
            f = ell(self.sqr(f), *l)
            if bit == "1":
                T, l = add(T, Q)
                f = ell(f, *l)
        if c.name == "bn254":
            gx, gy = self._pow2(c.xi, (c.q - 1) // 3), self._pow2(c.xi, (c.q - 1) // 2)
            cj = lambda a: (a[0], (-a[1]) % p)
            Q1 = (m(cj(Q[0]), gx), m(cj(Q[1]), gy))
            Q2 = (m(cj(Q1[0]), gx), f2_neg(m(cj(Q1[1]), gy), p))
            T, l = add(T, Q1)
            f = ell(f, *l)
            T, l = add(T, Q2)
            f = ell(f, *l)
        else:
            f = self.conj(f)
        return f

    # tower <-> flat
    def to_flat(self, a):
        out = [None] * 6
        for j in range(2):
            for i in range(3):
                out[2 * i + j] = a[j][i]
        return out

    def from_flat(self, a):
        return (tuple(a[2 * i] for i in range(3)), tuple(a[2 * i + 1] for i in range(3)))

    def random(self, rng: random.Random):
        return self.from_flat([(rng.randrange(self.p), rng.randrange(self.p)) for _ in range(6)])


@functools.lru_cache(maxsize=None)
def tower(name) -> Tower:
    return Tower(name)
