"""Exact reference and edge-case generator for the device arithmetic probe (tests/field_probe.py, tests/hip/).

Everything here is Python integer arithmetic: no device code, no oracle library; oracle/pyref only for the affine group law.
The saturated point arithmetic of ec_dev.hpp (EcOp) is checked against that group law alone.

An unsaturated element (unsat_dev.hpp) is L limbs of B bits; limbs 0..L-2 are < 2^B when "normalised", the top limb carries the
rest.  A value is not "an element below p" but "an integer below K*p"; the generator below puts operands at the top of the range
their call sites declare, and the checks compare the device's limbs with the one integer the operation must produce.

OPS maps an operation's name (as tests/hip spells it) to an Op:
    fields                    field names the operation is probed for
    cases(F, rng)             list of (in_words, out_init_words, ctx)
    nout(F)                   words per output row
    check(F, ctx, row)        raises AssertionError when the device's row is wrong
    pre(F, ctx)               raises AssertionError when the case violates the operation's precondition (CPU self-test)
    prods(F, ctx)             for product operations: the list of (a_limbs, b_limbs) the scan sums (column-sum self-test)
"""
from __future__ import annotations

import random
import re
from pathlib import Path

from oracle.pyref.curves import Group
from oracle.pyref.fields import BLS12_381, BN254

SEED = 0x5EED_F1E1D

# ------------------------------------------------------------------------------------------------------------ configuration
# Python copy of UnsatCfg<P> (unsat_dev.hpp); tests/test_field_ref.py compares it with the header text.
UNSAT_CFG = {
    "Bn254Fq": dict(L=9, B=29, MULCAP=160, CAPK=128),
    "Bn254Fr": dict(L=9, B=29, MULCAP=160, CAPK=128),
    "Bls381Fq": dict(L=14, B=28, MULCAP=2500, CAPK=2500),
    "Bls381Fr": dict(L=9, B=29, MULCAP=64, CAPK=64),
}
MODULI = {"Bn254Fq": (BN254.q, 8), "Bn254Fr": (BN254.r, 8), "Bls381Fq": (BLS12_381.q, 12), "Bls381Fr": (BLS12_381.r, 8)}
KMAX_TABLE = 48                                             # Fu::KMAX: multiples of p kept as limb tables


def parse_unsat_cfg(header_text: str) -> dict:
    """UnsatCfg<P> { L, B, MULCAP, CAPK } as the header states them."""
    out = {}
    for m in re.finditer(r"struct UnsatCfg<(\w+)> \{(.*?)\};", header_text, re.S):
        body = m.group(2)
        lb = re.search(r"L = (\d+), B = (\d+)", body)
        out[m.group(1)] = dict(L=int(lb.group(1)), B=int(lb.group(2)), MULCAP=int(re.search(r"MULCAP = (\d+)", body).group(1)),
                               CAPK=int(re.search(r"CAPK = (\d+)", body).group(1)))
    return out


class Field:
    def __init__(self, name: str):
        self.name = name
        self.p, self.N = MODULI[name]
        c = UNSAT_CFG[name]
        self.L, self.B, self.MULCAP, self.CAPK = c["L"], c["B"], c["MULCAP"], c["CAPK"]
        self.MASK = (1 << self.B) - 1
        self.R = 1 << (32 * self.N)                         # saturated Montgomery radix
        self.RP = 1 << (self.L * self.B)                    # unsaturated Montgomery radix R'
        self.SHIFT = self.L * self.B - 32 * self.N
        self.KIN = 1 << self.SHIFT                          # from_sat(X) = 2^SHIFT * X < KIN * p
        self.TOPSH = self.B * (self.L - 1)
        self.ninv = (-pow(self.p, -1, 1 << self.B)) % (1 << self.B)
        self.pinv_rp = pow(self.p, -1, self.RP)
        self.rp_inv = pow(self.RP, -1, self.p)
        self.r_inv = pow(self.R, -1, self.p)

    # ---- limbs
    def limbs(self, x: int) -> list:
        """Normalised limbs of x >= 0 (top limb unmasked, must fit 32 bits)."""
        assert 0 <= x < (1 << (self.TOPSH + 32)), "value does not fit the limbs"
        return [(x >> (self.B * i)) & self.MASK for i in range(self.L - 1)] + [x >> self.TOPSH]

    def val(self, limbs) -> int:
        return sum(int(l) << (self.B * i) for i, l in enumerate(limbs))

    def normalised(self, limbs) -> bool:
        return all(0 <= int(l) <= self.MASK for l in limbs[:-1]) and 0 <= int(limbs[-1]) < (1 << 32)

    def words(self, x: int) -> list:
        assert 0 <= x < self.R
        return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(self.N)]

    def from_words(self, ws) -> int:
        return sum(int(w) << (32 * i) for i, w in enumerate(ws))

    def mp(self, M: int) -> list:                           # Fu::mp_limb(M, .)
        return self.limbs(M * self.p)

    def lz(self, M: int) -> list:                           # Fu::lz_limb(M, .): redundant limbs of M * p
        mp = self.mp(M)
        return [mp[0] + (1 << self.B)] + [mp[i] + (1 << self.B) - 1 for i in range(1, self.L - 1)] + [mp[-1] - 1]

    def sub_lazy(self, M: int, a, b) -> list:               # limb model of Fu::sub_lazy<M>; neg_lazy<M> is a = 0
        lz = self.lz(M)
        r = [a[i] + lz[i] - b[i] for i in range(self.L)]
        assert all(lz[i] >= b[i] for i in range(self.L)) and all(0 <= x < (1 << 32) for x in r)
        return r

    # ---- Montgomery products
    def mont(self, prods) -> int:
        """The unique integer a product scan over sum a_i * b_i returns: (s + m p) / R' with m = -s p^-1 mod R'."""
        s = sum(a * b for a, b in prods)
        m = (-s * self.pinv_rp) % self.RP
        t = s + m * self.p
        assert t % self.RP == 0
        return t // self.RP

    def scan(self, prods):
        """Limb-by-limb model of Fu::mul / mul_add / mul_add4 (one 64-bit accumulator per column).  prods: (a_limbs, b_limbs)
        pairs.  Returns (result limbs, largest value the accumulator held)."""
        L, B, MASK = self.L, self.B, self.MASK
        pl = self.mp(1)
        m, r, acc, worst = [0] * L, [0] * L, 0, 0
        for k in range(2 * L - 1):
            for i in range(L):
                j = k - i
                if 0 <= j < L:
                    for a, b in prods:
                        acc += a[i] * b[j]
            for i in range(L):
                j = k - i
                if 0 <= j < L and i < k:
                    acc += m[i] * pl[j]
            if k < L:
                m[k] = (((acc & 0xFFFFFFFF) * self.ninv) & 0xFFFFFFFF) & MASK
                acc += m[k] * pl[0]
            else:
                r[k - L] = (acc & 0xFFFFFFFF) & MASK
            worst = max(worst, acc)
            acc >>= B
        r[L - 1] = acc & 0xFFFFFFFF
        return r, worst


FIELDS = {n: Field(n) for n in UNSAT_CFG}
ALL_FIELDS = list(FIELDS)
BASE_FIELDS = ["Bn254Fq", "Bls381Fq"]


# ------------------------------------------------------------------------------------------------------------ operand values
def edge_residues(F: Field) -> list:
    p, L, B, N = F.p, F.L, F.B, F.N
    out = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.R % p, F.RP % p, (F.RP - 1) % p]
    for i in range(1, L):
        out += [(1 << (B * i)) % p, ((1 << (B * i)) - 1) % p]
    for i in range(1, N):
        out += [(1 << (32 * i)) % p, ((1 << (32 * i)) - 1) % p]
    seen, res = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            res.append(c)
    return res


N_EXT = 4                                                   # the first N_EXT entries of reps() are the extremes of the range


def reps(F: Field, K: int, rng: random.Random, nrand: int = 24, extra=()) -> list:
    """Integers in [0, K*p): the extremes first (all-ones limbs below the top limb, K p - 1, zero limbs below the top limb, (K-1) p),
    then every edge residue c as c + j*p for j in {0, 1, K-1}."""
    p = F.p
    if K == 0:
        return [0]
    top = K * p - 1
    hi = top >> F.TOPSH
    ones = (hi << F.TOPSH) - 1 if hi else top               # every limb below the top all-ones
    zeros = hi << F.TOPSH                                   # every limb below the top zero
    vals = [ones, top, zeros, (K - 1) * p]
    for c in edge_residues(F) + [rng.randrange(p) for _ in range(nrand)]:
        for j in sorted({0, 1, K - 1}):
            if j < K:
                vals.append(c + j * p)
    vals += [v for v in extra if 0 <= v < K * p]
    seen, res = set(), []
    for v in vals:
        assert 0 <= v < K * p
        if v not in seen or len(res) < N_EXT:
            seen.add(v)
            res.append(v)
    return res


def combos(lists, n: int, rng: random.Random) -> list:
    """The full cross of the extremes of every list, then every entry of every list at least once, then random picks up to n."""
    out = []
    ext = [l[:min(2 if len(lists) > 4 else N_EXT, len(l))] for l in lists]
    idx = [0] * len(lists)
    while True:
        out.append(tuple(e[i] for e, i in zip(ext, idx)))
        k = 0
        while k < len(lists):
            idx[k] += 1
            if idx[k] < len(ext[k]):
                break
            idx[k] = 0
            k += 1
        if k == len(lists):
            break
    for t in range(max(len(l) for l in lists)):
        out.append(tuple(l[(t * (2 * k + 1) + k) % len(l)] for k, l in enumerate(lists)))
    while len(out) < n:
        out.append(tuple(rng.choice(l) for l in lists))
    return out


# Operand descriptors of the product operations:
#   ("n", K)        normalised limbs, value < K p
#   ("sl", M, KA)   lazy limbs of sub_lazy<M>(a, b), a < KA p, b < (M-1) p: value < (KA + M) p, limbs < 2^B + 2^(B+1)
#   ("nl", M)       lazy limbs of neg_lazy<M>(b), b < (M-1) p: value <= M p, limbs < 2^(B+1)
def desc_K(d) -> int:
    return d[1] if d[0] == "n" else d[2] + d[1] if d[0] == "sl" else d[1]


def operand_list(F: Field, d, rng: random.Random) -> list:
    """Limb lists for a descriptor, extremes first."""
    if d[0] == "n":
        return [F.limbs(v) for v in reps(F, d[1], rng, nrand=8)]
    M = d[1]
    B = reps(F, M - 1, rng, nrand=4)
    A = reps(F, d[2], rng, nrand=4) if d[0] == "sl" else [0]
    # as many limbs as possible at the top of the lazy range: a with all-ones low limbs, b with zero low limbs; then the largest
    # value (b = 0), then the rest
    pairs = [(A[0], B[2]), (A[min(1, len(A) - 1)], 0), (A[min(1, len(A) - 1)], B[2]), (A[0], 0)]
    for t in range(max(len(A), len(B))):
        pairs.append((A[t % len(A)], B[(3 * t + 1) % len(B)]))
    return [F.sub_lazy(M, F.limbs(a), F.limbs(b)) for a, b in pairs]


def flat(*parts) -> list:
    out = []
    for x in parts:
        out.extend(x)
    return out


class Op:
    fields = ALL_FIELDS

    def pre(self, F, ctx):
        pass


# ------------------------------------------------------------------------------------------------------------ Fp (saturated)
class FpOp(Op):
    """ctx = (operand integers, expected integer(s)); expected words are canonical."""

    def __init__(self, kind, fields=ALL_FIELDS):
        self.kind, self.fields = kind, fields

    def nout(self, F):
        return (2 if self.kind.startswith("fp2") else 1) * F.N

    def cases(self, F, rng):
        p, R, ri = F.p, F.R, F.r_inv
        A = reps(F, 1, rng, nrand=40)
        k = self.kind
        out = []
        if k in ("fp_add", "fp_sub", "fp_mul"):
            for a, b in combos([A, A], 1500, rng):
                e = (a + b) % p if k == "fp_add" else (a - b) % p if k == "fp_sub" else a * b * ri % p
                out.append((flat(F.words(a), F.words(b)), None, ((a, b), [e])))
        elif k == "fp_reduce_once":
            for a in reps(F, 2, rng, nrand=200):
                out.append((F.words(a), None, ((a,), [a % p])))
        elif k == "fp_pow_u64":
            E = [0, 1, 2, 3, 0xFFFFFFFF, 1 << 32, (1 << 64) - 1, 1 << 63] + [rng.getrandbits(64) for _ in range(8)]
            for a, e in combos([A, E], 300, rng):
                x = a * ri % p
                out.append((flat(F.words(a), [e & 0xFFFFFFFF, e >> 32]), None, ((a, e), [pow(x, e, p) * R % p])))
        elif k.startswith("fp2"):
            for a0, a1, b0, b1 in combos([A, A, A, A], 200 if k == "fp2_inv" else 1200, rng):
                x, y = (a0 * ri % p, a1 * ri % p), (b0 * ri % p, b1 * ri % p)
                if k == "fp2_mul":
                    e = ((x[0] * y[0] - x[1] * y[1]) % p, (x[0] * y[1] + x[1] * y[0]) % p)
                elif k == "fp2_sqr":
                    e = ((x[0] * x[0] - x[1] * x[1]) % p, 2 * x[0] * x[1] % p)
                else:
                    n = (x[0] * x[0] + x[1] * x[1]) % p
                    ni = pow(n, p - 2, p)
                    e = (x[0] * ni % p, -x[1] * ni % p)
                out.append((flat(F.words(a0), F.words(a1), F.words(b0), F.words(b1)), None,
                            ((a0, a1, b0, b1), [e[0] * R % p, e[1] * R % p])))
        else:
            for a in reps(F, 1, rng, nrand=300 if k == "fp_inv" else 1500):
                e = {"fp_neg": lambda: -a % p, "fp_dbl": lambda: 2 * a % p, "fp_sqr": lambda: a * a * ri % p,
                     "fp_to_mont": lambda: a * R % p, "fp_from_mont": lambda: a * ri % p,
                     "fp_inv": lambda: pow(a * ri % p, p - 2, p) * R % p}[k]()
                out.append((F.words(a), None, ((a,), [e])))
        return out

    def pre(self, F, ctx):
        ops = ctx[0]
        lim = 2 * F.p if self.kind == "fp_reduce_once" else F.p
        for a in (ops[:1] if self.kind == "fp_pow_u64" else ops):
            assert 0 <= a < lim

    def check(self, F, ctx, row):
        got = [F.from_words(row[i * F.N:(i + 1) * F.N]) for i in range(len(ctx[1]))]
        assert got == ctx[1], f"{self.kind}{tuple(hex(a) for a in ctx[0])}: got {[hex(g) for g in got]}, want {[hex(e) for e in ctx[1]]}"


# ------------------------------------------------------------------------------------------------------------ Fu products
def product_configs(F: Field, kind: str) -> list:
    """Operand descriptors per call: the factorisations the product's call sites use, and KA*KB (sums) at MULCAP exactly."""
    n = lambda K: ("n", K)
    cap, KIN = F.MULCAP, F.KIN
    big = F.name == "Bls381Fq"
    small = F.name == "Bls381Fr"
    if kind == "fu_mul":
        c = [(n(1), n(1)), (n(2), n(2)), (n(KIN), n(1)), (n(KIN), n(2)), (n(8), n(2)), (n(4), n(2)), (n(8), n(8)), (n(10), n(2)),
             (n(21), n(2)), (n(cap), n(1)), (n(cap // 2), n(2))]
        if not small:
            c += [(n(KIN), n(4) if not big else n(8)), (n(12), n(12)), (n(12), n(6)), (n(6), n(6)), (n(16), n(10))]
        if big:
            c += [(n(50), n(50)), (n(100), n(25))]
        return c
    if kind == "fu_sqr":
        c = [(n(1),), (n(2),), (n(4),), (n(6),), (n(8),)]
        if not small:
            c += [(n(10),), (n(12),)]
        if big:
            c += [(n(50),)]
        return c
    sl9, sl7, nl3, nl5, nl7 = ("sl", 9, 2), ("sl", 7, 2), ("nl", 3), ("nl", 5), ("nl", 7)
    if kind == "fu_mul_add":
        if small:                                           # MULCAP 64
            return [(n(4), sl9, n(4), nl5), (n(2), sl9, n(2), sl7), (n(2), sl9, n(4), sl7), (n(4), n(4), n(4), n(4)),
                    (n(2), n(2), n(2), nl3), (n(8), n(4), n(8), n(4))]
        c = [(n(8), sl9, n(4), nl3),                        # xyzz_madd_u y3: 8*11 + 4*3
             (n(4), sl9, n(2), nl3),                        # BkPoint add / add_mem / quad_add_mem y3
             (n(6), sl7, n(2), nl5),                        # BkPoint dbl y3: 6*9 + 2*5
             (n(KIN), n(2), n(KIN), nl3),                   # ub2_mul in xyzz_madd_u2: 32*2 + 32*3 = MULCAP for the 254-bit fields
             (n(KIN), n(2), n(KIN), n(2)),
             (n(4), n(2), n(4), nl3), (n(6), n(2), n(6), nl3), (n(2), n(2), n(2), nl3),
             (n(4), n(4), n(4), n(4)), (n(6), n(6), n(6), n(6)),   # sqr_lazy
             (n(2), n(2), n(0), n(0))]                      # the quad's spare lanes: c = d = 0
        if big:
            c += [(n(100), sl9, n(100), ("sl", 12, 2)), (n(50), n(25), n(50), n(25))]       # 1100 + 1400, 2500
        else:
            c += [(n(8), sl9, n(8), sl7)]                   # 88 + 72 = 160: two sub_lazy factors at MULCAP
        return c
    assert kind == "fu_mul_add4"
    if small:
        return [(n(4), n(4), n(4), ("nl", 4), n(4), n(4), n(4), n(4)), (n(2), n(2), n(2), nl3, n(2), n(2), n(2), n(2))]
    c = [(n(6), n(6), n(6), nl7, n(2), n(2), n(2), n(2)),   # y30 of xyzz_madd_u2 / add_mem / dbl_mem
         (n(6), n(6), n(6), n(6), n(2), nl3, n(2), n(2)),   # y31
         (n(4), n(6), n(4), nl7, n(2), n(2), n(2), n(2)),
         (n(4), n(6), n(4), n(6), n(2), n(2), n(2), n(2))]  # BkPoint<Fp2>::add / dbl: normalised negations
    if big:
        c += [(n(25), n(25), n(25), ("nl", 25), n(25), n(25), n(25), n(25))]
    else:
        c += [(n(8), n(8), n(8), ("nl", 8), n(4), n(4), n(4), n(4))]                        # 160 with one lazy factor
    return c


class FuProduct(Op):
    """ctx = (descriptors, operand limb lists)."""

    def __init__(self, kind):
        self.kind = kind

    def nout(self, F):
        return F.L

    def cases(self, F, rng):
        out = []
        cfgs = product_configs(F, self.kind)
        per = max(60, 2400 // len(cfgs))
        for cfg in cfgs:
            lists = [operand_list(F, d, rng) for d in cfg]
            for t in combos(lists, per, rng):
                out.append((flat(*t), None, (cfg, t)))
        return out

    def prods(self, F, ctx):
        t = ctx[1]
        if self.kind == "fu_sqr":
            return [(t[0], t[0])]
        return [(t[i], t[i + 1]) for i in range(0, len(t), 2)]

    def sum_kk(self, ctx):
        ks = [desc_K(d) for d in ctx[0]]
        if self.kind == "fu_sqr":
            return ks[0] * ks[0]
        return sum(ks[i] * ks[i + 1] for i in range(0, len(ks), 2))

    def pre(self, F, ctx):
        assert self.sum_kk(ctx) <= F.MULCAP, "sum of K products exceeds MULCAP"
        lazy_per_product = []
        for d, l in zip(*ctx):
            K = desc_K(d)
            assert K <= max(F.CAPK, F.MULCAP) and F.val(l) <= K * F.p
            if d[0] == "n":
                assert F.normalised(l) and F.val(l) < max(K, 1) * F.p
            else:
                assert d[1] <= KMAX_TABLE
                bound = (1 << F.B) + (1 << (F.B + 1)) if d[0] == "sl" else (1 << (F.B + 1))
                assert all(0 <= x < bound for x in l), "lazy limb above its stated bound"
        ds = ctx[0]
        if self.kind != "fu_sqr":
            for i in range(0, len(ds), 2):                  # "only ONE factor of a product whose other factor is normalised"
                lazy_per_product.append((ds[i][0] != "n") + (ds[i + 1][0] != "n"))
            assert max(lazy_per_product) <= 1
            if self.kind == "fu_mul_add4":
                assert sum(lazy_per_product) <= 1, "mul_add4 tolerates one lazy factor"

    def check(self, F, ctx, row):
        row = [int(x) for x in row]
        want = F.mont([(F.val(a), F.val(b)) for a, b in self.prods(F, ctx)])
        tag = f"{self.kind} {ctx[0]}"
        assert F.val(row) == want, f"{tag}: limbs spell {hex(F.val(row))}, want {hex(want)}; operands {ctx[1]}"
        assert F.normalised(row), f"{tag}: limbs not normalised: {row}"
        assert want < 2 * F.p, f"{tag}: result {hex(want)} >= 2p with sum KK = {self.sum_kk(ctx)} <= MULCAP"


# ------------------------------------------------------------------------------------------------------------ Fu add / sub
class FuLinear(Op):
    """ctx = (operand integers, m).  kinds: add, dbl, sub<M>, sub_sub2<M>, sub_sel<M>, csub<M>, sub_lazy<M>, neg_lazy<M>."""
    # (KA, ...) bounds the call sites use
    CFG = {
        "fu_add": [(2, 2), (4, 4), (6, 6), (4, 2), (1, 1), ("half", "half")],
        "fu_dbl": [(1,), (2,), (4,), (6,), (8,), ("half",)],
        "fu_sub<2>": [(2, 2), (6, 2), (21, 2), (4, 2)],     # ntt.hip: a up to 21p
        "fu_sub<4>": [(2, 4), (4, 4), (6, 4), (0, 4)],
        "fu_sub<6>": [(0, 6), (6, 6), (2, 6)],
        "fu_sub<8>": [(2, 8), (0, 8)],
        "fu_sub_sub2<6>": [(2, 2, 2), (4, 2, 2)],
        "fu_sub_sel<2>": [(2, 0), (1, 1)],
        "fu_sub_sel<4>": [(2, 2)],
        "fu_sub_sel<6>": [(2, 4)],
        "fu_csub<2>": [(4,)],
        "fu_csub<4>": [(8,)],
        "fu_sub_lazy<7>": [(2, 6)],
        "fu_sub_lazy<9>": [(2, 8)],
        "fu_neg_lazy<3>": [(2,)],
        "fu_neg_lazy<5>": [(4,)],
        "fu_neg_lazy<7>": [(6,)],
    }

    def __init__(self, kind):
        self.kind = kind
        m = re.search(r"<(\d+)>", kind)
        self.M = int(m.group(1)) if m else 0
        self.base = kind.split("<")[0]

    def nout(self, F):
        return F.L

    def cases(self, F, rng):
        out, M, p = [], self.M, F.p
        cfgs = self.CFG[self.kind]
        per = max(300, 2400 // len(cfgs))
        for cfg in cfgs:
            cfg = tuple(F.CAPK // 2 if k == "half" else k for k in cfg)
            extra = [M * p - 1, M * p, M * p + 1] if self.base == "fu_csub" else ()
            lists = [reps(F, K, rng, nrand=12, extra=extra) for K in cfg]
            if self.base == "fu_sub_sel":
                lists.append([0, 0xFFFFFFFF])
            for t in combos(lists, per, rng):
                m = 0
                if self.base == "fu_sub_sel":
                    t, m = t[:-1], t[-1]
                if self.base == "fu_sub_sub2" and t[1] + 2 * t[2] >= M * p:
                    continue                                # cannot happen for (.., 2, 2) with M = 6
                words = flat(*[F.limbs(v) for v in t]) + ([m] if self.base == "fu_sub_sel" else [])
                out.append((words, None, (cfg, t, m)))
        return out

    def pre(self, F, ctx):
        cfg, t, m = ctx
        M, p, b = self.M, F.p, self.base
        for K, v in zip(cfg, t):
            assert 0 <= v < max(K, 1) * p and (K > 0 or v == 0)
            F.limbs(v)
        if b == "fu_sub":
            assert t[1] < M * p
        elif b == "fu_sub_sub2":
            assert t[1] + 2 * t[2] < M * p
        elif b == "fu_sub_sel":
            assert t[0] + t[1] < M * p and m in (0, 0xFFFFFFFF)
        elif b == "fu_csub":
            assert t[0] < 2 * M * p and (t[0] >> F.TOPSH) < (1 << 31)
        elif b == "fu_sub_lazy":
            assert t[1] < (M - 1) * p
        elif b == "fu_neg_lazy":
            assert t[0] < (M - 1) * p
        elif b in ("fu_add", "fu_dbl"):
            assert sum(cfg) * (2 if b == "fu_dbl" else 1) <= F.CAPK

    def check(self, F, ctx, row):
        cfg, t, m = ctx
        row = [int(x) for x in row]
        M, p, b = self.M, F.p, self.base
        lazy_bound = None
        if b == "fu_add":
            want, hi = t[0] + t[1], sum(cfg) * p
        elif b == "fu_dbl":
            want, hi = 2 * t[0], 2 * cfg[0] * p
        elif b == "fu_sub":
            want, hi = t[0] - t[1] + M * p, (cfg[0] + M) * p + (cfg[0] == 0)     # ub_neg<M>(0) is M p itself
        elif b == "fu_sub_sub2":
            want, hi = t[0] - t[1] - 2 * t[2] + M * p, (cfg[0] + M) * p
        elif b == "fu_sub_sel":
            want, hi = (-t[0] if m else t[0]) - t[1] + M * p, (2 * cfg[0] + cfg[1]) * p + 1
        elif b == "fu_csub":
            want, hi = (t[0] - M * p if t[0] >= M * p else t[0]), M * p
        elif b == "fu_sub_lazy":
            want, hi, lazy_bound = t[0] - t[1] + M * p, (cfg[0] + M) * p, (1 << F.B) + (1 << (F.B + 1))
        else:
            want, hi, lazy_bound = M * p - t[0], M * p + 1, 1 << (F.B + 1)
        tag = f"{self.kind} {cfg} m={m:#x} operands {[hex(v) for v in t]}"
        assert F.val(row) == want, f"{tag}: limbs spell {hex(F.val(row))}, want {hex(want)}"
        if lazy_bound is None:
            assert F.normalised(row), f"{tag}: limbs not normalised: {row}"
        else:
            assert all(0 <= x < lazy_bound for x in row), f"{tag}: lazy limb above {lazy_bound:#x}: {row}"
        lo = 0 if b in ("fu_add", "fu_dbl", "fu_csub") else 1
        assert lo <= want < hi, f"{tag}: value outside the promised range"


# ------------------------------------------------------------------------------------------------------------ Fu conversions
class FuConv(Op):
    def __init__(self, kind):
        self.kind = kind

    def nout(self, F):
        return F.N if self.kind in ("fu_to_words", "fu_to_sat", "fu_ntt_mul") else F.L

    def cases(self, F, rng):
        k, p, out = self.kind, F.p, []
        if k == "fu_from_words":                            # any 32N-bit value, not only residues
            top = F.R - 1
            V = reps(F, 1, rng, nrand=300) + [top, top - 1, F.R >> 1, (F.R >> 1) - 1] + [rng.getrandbits(32 * F.N) for _ in range(300)]
            for i in range(1, F.L):                         # all-ones below / above every limb boundary
                low = (1 << (F.B * i)) - 1
                V += [low & top, top ^ (low & top)]
            return [(F.words(v), None, (v,)) for v in V]
        if k in ("fu_from_sat", "fu_from_sat_reduced"):
            return [(F.words(v), None, (v,)) for v in reps(F, 1, rng, nrand=1500)]
        if k == "fu_to_words":
            V = reps(F, 2, rng, nrand=300) + [F.R - 1, F.R - 2, F.R >> 1] + [rng.getrandbits(32 * F.N) for _ in range(600)]
            return [(F.limbs(v), None, (v,)) for v in V]
        if k == "fu_to_sat":
            for K in (1, 2, 4, 8, 64):                      # "any value < 64p"
                out += [(F.limbs(v), None, (v, K)) for v in reps(F, K, rng, nrand=100)]
            return out
        if k == "fu_one":
            return [([0], None, ())]
        assert k == "fu_ntt_mul"
        X = reps(F, 1, rng, nrand=16)
        for K in (1, 2, F.KIN):                             # twiddles < p, products < 2p, from_sat(s) < 2^SHIFT p
            for x, t in combos([X, reps(F, K, rng, nrand=16)], 800, rng):
                out.append((flat(F.words(x), F.limbs(t)), None, (x, t, K)))
        return out

    def pre(self, F, ctx):
        k = self.kind
        if k == "fu_from_words":
            assert ctx[0] < F.R
        elif k in ("fu_from_sat", "fu_from_sat_reduced"):
            assert ctx[0] < F.p and F.KIN * 1 <= F.MULCAP
        elif k == "fu_to_words":
            assert ctx[0] < F.R
        elif k == "fu_to_sat":
            assert ctx[0] < ctx[1] * F.p and ctx[1] * 1 <= F.MULCAP
        elif k == "fu_ntt_mul":
            assert ctx[0] < F.p and ctx[1] < ctx[2] * F.p and ctx[2] <= F.MULCAP

    def check(self, F, ctx, row):
        row = [int(x) for x in row]
        k, p = self.kind, F.p
        tag = f"{k} {tuple(hex(c) for c in ctx)}"
        if k in ("fu_from_words", "fu_from_sat", "fu_from_sat_reduced", "fu_one"):
            if k == "fu_from_words":
                want = ctx[0]
            elif k == "fu_from_sat":
                want = ctx[0] << F.SHIFT
            elif k == "fu_from_sat_reduced":
                want = F.mont([(ctx[0] << F.SHIFT, F.RP % p)])
                assert want < 2 * p
            else:
                want = F.RP % p
            assert F.val(row) == want, f"{tag}: limbs spell {hex(F.val(row))}, want {hex(want)}"
            assert F.normalised(row) and (k == "fu_from_sat_reduced" or row[-1] <= F.MASK), f"{tag}: limbs not normalised: {row}"
            return
        got = F.from_words(row)
        if k == "fu_to_words":
            want = ctx[0]
        elif k == "fu_to_sat":
            want = ctx[0] * F.rp_inv * F.R % p
        else:
            want = ctx[0] * ctx[1] * F.rp_inv % p
        assert got == want, f"{tag}: got {hex(got)}, want {hex(want)}"


class FuPred(Op):
    """ctx = (value, K)."""

    def __init__(self, kind, K):
        self.kind, self.K, self.base = kind, K, kind.split("<")[0]

    def nout(self, F):
        return 1

    def cases(self, F, rng):
        K, p = self.K, F.p
        low2 = 1 << (2 * F.B)
        V = []
        for k in range(K):
            V += [v for v in (k * p, k * p - 1, k * p + 1) if 0 <= v < K * p]
            for _ in range(40):                             # the two low limbs of k p, other limbs different
                v = (k * p) % low2 + low2 * rng.randrange((K * p) >> (2 * F.B))
                if v < K * p:
                    V.append(v)
            for i in range(2, F.L):                         # k p with one bit flipped in limb i
                v = (k * p) ^ (1 << (F.B * i + rng.randrange(F.B if i < F.L - 1 else 8)))
                if v < K * p:
                    V.append(v)
        V += reps(F, K, rng, nrand=200)
        return [(F.limbs(v), None, (v, K)) for v in V]

    def pre(self, F, ctx):
        assert 0 <= ctx[0] < ctx[1] * F.p

    def check(self, F, ctx, row):
        v, K = ctx
        p = F.p
        low2 = 1 << (2 * F.B)
        if self.base == "fu_is_zero_mod_p":
            want = v % p == 0
        elif self.base == "fu_is_multiple_of_p":
            want = v % p == 0 and v != 0
        else:
            want = any(v % low2 == (k * p) % low2 for k in range(1, K))
        assert int(row[0]) == int(want), f"{self.kind}({hex(v)}): got {int(row[0])}, want {int(want)}"


# ------------------------------------------------------------------------------------------------------------ points
def f2_sqrt(a, p):
    """Square root in Fq[u]/(u^2 + 1), p = 3 (mod 4); None if a is not a square."""
    def mul(x, y):
        return ((x[0] * y[0] - x[1] * y[1]) % p, (x[0] * y[1] + x[1] * y[0]) % p)

    def fpow(x, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = mul(r, x)
            x = mul(x, x)
            e >>= 1
        return r
    if a == (0, 0):
        return (0, 0)
    a1 = fpow(a, (p - 3) // 4)
    alpha = mul(mul(a1, a1), a)
    a0 = mul((alpha[0], -alpha[1] % p), alpha)
    if a0 == (p - 1, 0):
        return None
    x0 = mul(a1, a)
    if alpha == (p - 1, 0):
        r = mul((0, 1), x0)
    else:
        b = fpow(((1 + alpha[0]) % p, alpha[1]), (p - 1) // 2)
        r = mul(b, x0)
    return r if mul(r, r) == a else None


class PointLayer:
    """Group g (1 / 2) over base field F: bucket points as limbs <-> affine points of oracle/pyref."""

    def __init__(self, F: Field, g: int):
        self.F, self.g = F, g
        self.G = Group(BN254 if F.name == "Bn254Fq" else BLS12_381, g)
        self.KX, self.KY = (8, 4) if g == 1 else (4, 2)     # stored bounds: x < 8p / 4p, y < 4p / 2p, zz, zzz < 2p
        self.BOUNDS = (self.KX, self.KY, 2, 2)
        self.PT = 4 * g * F.L                               # words of a bucket point
        self.SAT = 4 * g * F.N                              # words of a saturated XYZZ point

    def comps(self, c):
        return (c,) if self.g == 1 else tuple(c)

    def elt(self, t):
        return t[0] if self.g == 1 else tuple(t)

    def rand_elt(self, rng):
        return self.elt([rng.randrange(1, self.F.p) for _ in range(self.g)])

    # ---- affine points
    def point_from_x(self, x):
        """(x, y) on the curve, or None."""
        Fo, p = self.G.F, self.F.p
        rhs = Fo.add(Fo.mul(Fo.sqr(x), x), self.G.b)
        if self.g == 1:
            y = pow(rhs, (p + 1) // 4, p)
            ok = y * y % p == rhs
        else:
            y = f2_sqrt(rhs, p)
            ok = y is not None
        if not ok or Fo.is_zero(y):
            return None
        return (x, y)

    def search_point(self, xm_comps):
        """Walk the Montgomery-form x (saturated radix) downward from a pattern until x is on the curve."""
        F = self.F
        xm = list(xm_comps)
        for _ in range(2000):
            x = self.elt([c * F.r_inv % F.p for c in xm])
            P = self.point_from_x(x)
            if P is not None:
                return P
            xm[0] -= 1
        raise AssertionError("no curve point near the pattern")

    def affine_points(self, rng, nrand=6):
        """Random multiples of the generator, the generator, and points whose Montgomery-form x has extreme limbs."""
        F, G = self.F, self.G
        pts = [G.gen] + [G.mul(G.gen, rng.randrange(1, G.order)) for _ in range(nrand)]
        w = 32 * (F.N - 1)
        hi = (F.p - 1) >> w
        pats = [F.p - 1, ((hi - 1) << w) | ((1 << w) - 1), hi << w, (1 << w) - 1, 1 << w, F.R % F.p]
        for i, a in enumerate(pats):
            other = pats[(i + 1) % len(pats)]
            P = self.search_point([a] if self.g == 1 else [a, other])
            pts.append(P)
            pts.append(G.neg(P) if i % 2 else P)
        return pts

    # ---- representations
    def acc_coords(self, P, z, mode, rng, bounds=None):
        """(X z^2, Y z^3, z^2, z^3) in unsaturated Montgomery form, every component lifted inside its declared bound:
        mode 'low' -> below p, 'top' -> the top representative, 'rand' -> a random one."""
        F, Fo = self.F, self.G.F
        z2 = Fo.sqr(z)
        z3 = Fo.mul(z2, z)
        plain = [Fo.mul(P[0], z2), Fo.mul(P[1], z3), z2, z3]
        out = []
        modes = (mode,) * 4 if isinstance(mode, str) else mode     # one mode, or one per coordinate
        for c, K, md in zip(plain, bounds or self.BOUNDS, modes):
            t = []
            for ci in self.comps(c):
                v = ci * F.RP % F.p
                j = 0 if md == "low" else K - 1 if md == "top" else rng.randrange(K)
                t.append(v + j * F.p)
            out.append(tuple(t))
        return out

    def cross(self, a, b):
        """The integers the device gets for a * b, a a coordinate (x or y) and b a zz / zzz below 2p: Fu::mul for G1, the two
        lazily reduced sums of ub2_mul (c0 = a0 b0 + a1 (3p - b1), c1 = a0 b1 + a1 b0) for G2."""
        F = self.F
        if self.g == 1:
            return (F.mont([(a[0], b[0])]),)
        return (F.mont([(a[0], b[0]), (a[1], 3 * F.p - b[1])]), F.mont([(a[0], b[1]), (a[1], b[0])]))

    def same_point_pair(self, P, negate, which, k, rng, tries=20000):
        """Representations a of P and b of +-P for which the device's x-difference u2 - u1 + 2p (which = 0) or y-difference
        (which = 1) has a component that is exactly k p, k = 1 or 3: the ends of the range is_multiple_of_p<4> has to cover.
        Random representations give 2p almost always (a product leaves the scan at or above p once in a hundred)."""
        Q = self.G.neg(P) if negate else P
        hi, lo = ("top", "low") if k == 3 else ("low", "top")
        ma = tuple(lo if i == which else hi if i == which + 2 else "rand" for i in range(4))   # u1 = a.x b.zz small, u2 = b.x a.zz large
        mb = tuple(hi if i == which else lo if i == which + 2 else "rand" for i in range(4))
        for _ in range(tries):
            a = self.acc_coords(P, self.rand_elt(rng), ma, rng)
            b = self.acc_coords(Q, self.rand_elt(rng), mb, rng)
            u1, u2 = self.cross(a[which], b[which + 2]), self.cross(b[which], a[which + 2])
            d = [y - x + 2 * self.F.p for x, y in zip(u1, u2)]
            if any(v == k * self.F.p for v in d):
                assert all(v % self.F.p == 0 for v in d)
                return a, b
        raise AssertionError("no representation found")

    def identity(self):
        return [tuple([0] * self.g)] * 4

    def point_words(self, coords):
        return flat(*[self.F.limbs(v) for c in coords for v in c])

    def sat_words(self, P, z):
        """Saturated XYZZ words (canonical Montgomery, radix 2^(32N)) of P scaled by z; P None -> the identity (1, 1, 0, 0)."""
        F, Fo = self.F, self.G.F
        if P is None:
            plain = [Fo.one, Fo.one, Fo.zero, Fo.zero]
        else:
            z2 = Fo.sqr(z)
            z3 = Fo.mul(z2, z)
            plain = [Fo.mul(P[0], z2), Fo.mul(P[1], z3), z2, z3]
        return flat(*[F.words(ci * F.R % F.p) for c in plain for ci in self.comps(c)]), plain

    def affine_words(self, P):
        F = self.F
        return flat(*[F.words(ci * F.R % F.p) for c in P for ci in self.comps(c)])

    def decode(self, row):
        F, g = self.F, self.g
        row = [int(x) for x in row]
        return [tuple(row[(k * g + i) * F.L:(k * g + i + 1) * F.L] for i in range(g)) for k in range(4)]

    def affine_of(self, coords_int):
        """Affine point a bucket point (integers, unsaturated Montgomery) stands for; None for zz == 0 (mod p)."""
        F, Fo = self.F, self.G.F
        x, y, zz, zzz = [self.elt([v * F.rp_inv % F.p for v in c]) for c in coords_int]
        if Fo.is_zero(zz):
            return None
        assert Fo.mul(Fo.sqr(zz), zz) == Fo.sqr(zzz), "zz^3 != zzz^2"
        return (Fo.mul(x, Fo.inv(zz)), Fo.mul(y, Fo.inv(zzz)))

    def check_point(self, row, want, tag, bounds=None):
        """The device's bucket point `row` is `want` (affine, None = identity: all-zero limbs) within the stored bounds."""
        F = self.F
        limbs = self.decode(row[:self.PT])
        if want is None:
            assert all(l == 0 for c in limbs for comp in c for l in comp), f"{tag}: identity expected, got {limbs}"
            return
        names = ("x", "y", "zz", "zzz")
        ints = []
        for name, c, K in zip(names, limbs, bounds or self.BOUNDS):
            for comp in c:
                assert F.normalised(comp), f"{tag}: {name} limbs not normalised: {comp}"
                assert F.val(comp) < K * F.p, f"{tag}: {name} = {hex(F.val(comp))} is not below {K}p"
            ints.append(tuple(F.val(comp) for comp in c))
        got = self.affine_of(ints)
        assert got == want, f"{tag}: point is {got}, want {want}"


LAYERS = {}


def layer(fname: str, g: int) -> PointLayer:
    if (fname, g) not in LAYERS:
        LAYERS[(fname, g)] = PointLayer(FIELDS[fname], g)
    return LAYERS[(fname, g)]


def pair_cases(PL: PointLayer, rng, n_generic):
    """(kind, a_coords, b_coords, expected affine) for a + b over bucket points: generic, identity on either side, P = Q, P = -Q,
    the last two also as different representatives of the same coordinates."""
    G = PL.G
    pts = PL.affine_points(rng)
    out = []
    modes = ("low", "top", "rand")
    for i in range(n_generic):
        P, Q = pts[i % len(pts)], pts[(i * 5 + 3) % len(pts)]
        if P[0] == Q[0]:
            Q = G.add(Q, G.gen) if G.add(Q, G.gen) is not None and G.add(Q, G.gen)[0] != P[0] else G.mul(G.gen, 7)
        ma, mb = modes[i % 3], modes[(i // 3) % 3]
        out.append(("generic", PL.acc_coords(P, PL.rand_elt(rng), ma, rng), PL.acc_coords(Q, PL.rand_elt(rng), mb, rng), G.add(P, Q)))
    for i, P in enumerate(pts):
        m = modes[i % 3]
        a = PL.acc_coords(P, PL.rand_elt(rng), m, rng)
        out.append(("b=identity", a, PL.identity(), P))
        out.append(("a=identity", PL.identity(), a, P))
        z = PL.rand_elt(rng)
        # the same representation on both sides: pd is exactly 2p
        out.append(("P=Q same rep", PL.acc_coords(P, z, m, rng), PL.acc_coords(P, z, m, rng), G.add(P, P)))
        out.append(("P=-Q same z", PL.acc_coords(P, z, m, rng), PL.acc_coords(G.neg(P), z, m, rng), None))
        for m2 in modes:                                    # different z, different lifts: pd is p, 2p or 3p
            out.append(("P=Q other rep", PL.acc_coords(P, PL.rand_elt(rng), m, rng), PL.acc_coords(P, PL.rand_elt(rng), m2, rng), G.add(P, P)))
            out.append(("P=-Q other rep", PL.acc_coords(P, PL.rand_elt(rng), m, rng), PL.acc_coords(G.neg(P), PL.rand_elt(rng), m2, rng), None))
    for P in pts[:4]:                                       # pd / rd at the ends of {p, 2p, 3p}
        for k in (1, 3):
            a, b = PL.same_point_pair(P, False, 0, k, rng)
            out.append((f"P=Q pd={k}p", a, b, G.add(P, P)))
            a, b = PL.same_point_pair(P, True, 0, k, rng)
            out.append((f"P=-Q pd={k}p", a, b, None))
            a, b = PL.same_point_pair(P, False, 1, k, rng)
            out.append((f"P=Q rd={k}p", a, b, G.add(P, P)))
    out.append(("both identity", PL.identity(), PL.identity(), None))
    return out


class PointOp(Op):
    fields = BASE_FIELDS

    def __init__(self, kind, g, fields=BASE_FIELDS):
        self.kind, self.g, self.fields = kind, g, fields

    def PL(self, F):
        return layer(F.name, self.g)


class MaddOp(PointOp):
    """xyzz_madd_u / xyzz_madd_u2 followed by the degenerate predicate.  ctx = (kind, expected affine or 'degenerate')."""

    def nout(self, F):
        return self.PL(F).PT + 3

    def cases(self, F, rng):
        PL, G = self.PL(F), self.PL(F).G
        pts = PL.affine_points(rng)
        out = []
        modes = ("low", "top", "rand")

        def add(kind, acc, inf, P, negm, want):
            words = flat(PL.point_words(acc), [inf], PL.affine_words(P), [negm])
            out.append((words, None, (kind, want, inf)))
        # acc.inf with the top of sub_sel<2>'s range: points whose y * one comes out of the product scan at or above p (one in
        # forty to a hundred random points), so that -y + 2p and a wrong multiple of p differ
        Q, high = G.gen, []
        for _ in range(8000):
            Q = G.add(Q, G.gen)
            if any(F.mont([((c * F.R % F.p) << F.SHIFT, F.RP % F.p)]) >= F.p for c in PL.comps(Q[1])):
                high.append(Q)
                if len(high) == 8:
                    break
        assert len(high) == 8
        for A in high:
            for negm in (0, 0xFFFFFFFF):
                add("acc.inf, y*one >= p", PL.identity(), 1, A, negm, G.neg(A) if negm else A)
        t = 0
        for i, A in enumerate(pts):
            for k in range(6):
                P = pts[(i * 3 + k + 1) % len(pts)]
                if P[0] == A[0]:
                    continue
                negm = 0xFFFFFFFF if (t // 3) % 2 else 0
                add("generic", PL.acc_coords(A, PL.rand_elt(rng), modes[t % 3], rng), 0, P, negm, G.add(A, G.neg(P) if negm else P))
                t += 1
            for negm in (0, 0xFFFFFFFF):
                add("acc.inf", PL.identity(), 1, A, negm, G.neg(A) if negm else A)
                for m in modes:                             # P = +-acc is part of the contract: the predicate must fire afterwards
                    add("P=acc", PL.acc_coords(A, PL.rand_elt(rng), m, rng), 0, A, negm, "degenerate")
                    add("P=-acc", PL.acc_coords(G.neg(A), PL.rand_elt(rng), m, rng), 0, A, negm, "degenerate")
        return out

    def check(self, F, ctx, row):
        PL = self.PL(F)
        kind, want, inf = ctx
        tag = f"{self.kind} [{kind}]"
        inf_out, ret, deg = int(row[PL.PT]), int(row[PL.PT + 1]), int(row[PL.PT + 2])
        assert ret == 1 and inf_out == 0, f"{tag}: returned {ret}, acc.inf {inf_out}"
        if want == "degenerate":
            assert deg == 1, f"{tag}: the degenerate predicate did not fire"
            return
        assert deg == 0, f"{tag}: the degenerate predicate fired on a regular addition"
        PL.check_point(row, want, tag)


class BkConvOp(PointOp):
    """BkPoint::from_sat / to_sat."""

    def nout(self, F):
        return self.PL(F).PT if self.kind.endswith("from_sat") else self.PL(F).SAT + 1

    def cases(self, F, rng):
        PL = self.PL(F)
        pts = PL.affine_points(rng)
        out = []
        if self.kind.endswith("from_sat"):
            for i in range(120):
                w, plain = PL.sat_words(pts[i % len(pts)], PL.rand_elt(rng))
                out.append((w, None, plain))
            for P in pts:
                w, plain = PL.sat_words(P, PL.G.F.one)
                out.append((w, None, plain))
            out.append((PL.sat_words(None, None)[0], None, None))
        else:
            modes = ("low", "top", "rand")
            for i in range(150):
                c = PL.acc_coords(pts[i % len(pts)], PL.rand_elt(rng), modes[i % 3], rng)
                out.append((PL.point_words(c), None, c))
            out.append((PL.point_words(PL.identity()), None, None))
        return out

    def check(self, F, ctx, row):
        PL, p = self.PL(F), F.p
        row = [int(x) for x in row]
        if self.kind.endswith("from_sat"):
            limbs = PL.decode(row)
            if ctx is None:
                assert all(l == 0 for c in limbs for comp in c for l in comp), f"{self.kind}: identity expected"
                return
            for name, c, plain in zip(("x", "y", "zz", "zzz"), limbs, ctx):
                for comp, ci in zip(c, PL.comps(plain)):
                    want = F.mont([((ci * F.R % p) << F.SHIFT, F.RP % p)])      # from_sat_reduced: exact integer, < 2p
                    assert F.val(comp) == want and F.normalised(comp) and want < 2 * p, f"{self.kind}: {name} = {comp}, want {hex(want)}"
            return
        sat = [F.from_words(row[i * F.N:(i + 1) * F.N]) for i in range(4 * self.g)]
        flag = row[PL.SAT]
        if ctx is None:
            one = F.R % p
            want = flat(*[[one] + [0] * (self.g - 1)] * 2) + [0] * (2 * self.g)
            assert flag == 1 and sat == want, f"{self.kind}: identity expected, got {sat}, flag {flag}"
            return
        want = [v * F.rp_inv * F.R % p for c in ctx for v in c]
        assert flag == 0 and sat == want, f"{self.kind}: got {[hex(s) for s in sat]}, want {[hex(s) for s in want]}"


class BkAddOp(PointOp):
    """BkPoint::add (registers), add_mem / quad_add_mem / quad_add_mem2 (memory, out distinct / over a / over b).
    ctx = (kind, expected affine, mode, a words, b words)."""
    MEM = False

    def nout(self, F):
        return (3 if self.MEM else 1) * self.PL(F).PT

    def cases(self, F, rng):
        PL = self.PL(F)
        out = []
        for i, (kind, a, b, want) in enumerate(pair_cases(PL, rng, 120)):
            aw, bw = PL.point_words(a), PL.point_words(b)
            if not self.MEM:
                out.append((flat(aw, bw), None, (kind, want, 0, aw, bw)))
            else:
                for mode in ((0, 1, 2) if kind != "generic" else (i % 3,)):
                    out.append(([mode], flat(aw, bw, [0xDEADBEEF] * PL.PT), (kind, want, mode, aw, bw)))
        return out

    def result(self, F, ctx, row):
        PT = self.PL(F).PT
        if not self.MEM:
            return row[:PT]
        mode = ctx[2]
        s = 0 if mode == 1 else PT if mode == 2 else 2 * PT
        return row[s:s + PT]

    def check(self, F, ctx, row):
        PL = self.PL(F)
        kind, want, mode, aw, bw = ctx
        tag = f"{self.kind} [{kind}, out mode {mode}]"
        row = [int(x) for x in row]
        if self.MEM:                                        # operands that are not the destination stay as they were
            if mode != 1:
                assert row[:PL.PT] == aw, f"{tag}: operand a was overwritten"
            if mode != 2:
                assert row[PL.PT:2 * PL.PT] == bw, f"{tag}: operand b was overwritten"
        # sums are stored with y < 2p for G1 too (y3 is a fresh product); copies of an operand keep the operand's bound
        PL.check_point(self.result(F, ctx, row), want, tag)


class BkAddMemOp(BkAddOp):
    MEM = True


class BkDblOp(PointOp):
    """BkPoint::dbl (registers), dbl_mem / quad_dbl_mem (memory, out distinct / in place).  ctx = (kind, expected, mode, a words)."""
    MEM = False

    def __init__(self, kind, g, fields=BASE_FIELDS, identity=True):
        super().__init__(kind, g, fields)
        self.identity = identity

    def nout(self, F):
        return (3 if self.MEM else 1) * self.PL(F).PT

    def cases(self, F, rng):
        PL = self.PL(F)
        pts = PL.affine_points(rng)
        modes = ("low", "top", "rand")
        out = []
        items = [(pts[i % len(pts)], modes[i % 3]) for i in range(150)] + ([(None, "low")] if self.identity else [])
        for i, (P, m) in enumerate(items):
            a = PL.identity() if P is None else PL.acc_coords(P, PL.rand_elt(rng), m, rng)
            aw = PL.point_words(a)
            want = None if P is None else PL.G.add(P, P)
            if not self.MEM:
                out.append((aw, None, ("dbl", want, 0, aw)))
            else:
                for mode in (0, 1):
                    out.append(([mode], flat(aw, [0xDEADBEEF] * (2 * PL.PT)), ("dbl", want, mode, aw)))
        return out

    def result(self, F, ctx, row):
        PT = self.PL(F).PT
        s = 0 if (not self.MEM or ctx[2] == 1) else 2 * PT
        return row[s:s + PT]

    def check(self, F, ctx, row):
        PL = self.PL(F)
        row = [int(x) for x in row]
        tag = f"{self.kind} [out mode {ctx[2]}]"
        if self.MEM and ctx[2] == 0:
            assert row[:PL.PT] == ctx[3], f"{tag}: operand was overwritten"
        PL.check_point(self.result(F, ctx, row), ctx[1], tag)


class BkDblMemOp(BkDblOp):
    MEM = True


# ------------------------------------------------------------------------------------------------------------ ec_dev.hpp
class EcOp(PointOp):
    """XYZZ<F> of ec_dev.hpp on canonical saturated Montgomery words, one method per operation.  The reference is the affine group
    law of oracle/pyref in Python integers; a result is compared as a GROUP ELEMENT (x / zz, y / zzz after normalising here), every
    stored coordinate must be canonical (below p) and every non-identity result must keep zz^3 == zzz^2.  The identity is zz == 0.
    ctx = (case class, expected affine point or None, extra)."""
    KINDS = ("dbl_affine", "dbl", "madd", "madd_fast", "add", "to_affine", "store_jacobian", "from_jacobian")

    def __init__(self, kind, g, fields=BASE_FIELDS):
        super().__init__(kind, g, fields)
        self.base = kind.split("_", 1)[1]
        assert self.base in self.KINDS

    def W(self, F):
        return self.g * F.N

    def nout(self, F):
        W = self.W(F)
        return {"to_affine": 2 * W, "store_jacobian": 3 * W, "madd_fast": 4 * W + 1}.get(self.base, 4 * W)

    # ---- words <-> field elements
    def enc(self, F, *elts):
        return flat(*[F.words(ci * F.R % F.p) for c in elts for ci in self.PL(F).comps(c)])

    def dec(self, F, row, n, tag):
        PL, W = self.PL(F), self.W(F)
        out = []
        for k in range(n):
            raw = [F.from_words(row[k * W + i * F.N:k * W + (i + 1) * F.N]) for i in range(self.g)]
            assert all(v < F.p for v in raw), f"{tag}: coordinate {k} is not canonical: {[hex(v) for v in raw]}"
            out.append(PL.elt([v * F.r_inv % F.p for v in raw]))
        return out

    def xyzz(self, F, P, z):
        """(x z^2, y z^3, z^2, z^3) as field elements."""
        Fo = self.PL(F).G.F
        z2 = Fo.sqr(z)
        z3 = Fo.mul(z2, z)
        return [Fo.mul(P[0], z2), Fo.mul(P[1], z3), z2, z3]

    def identities(self, F, rng):
        """The forms of the identity: inf() = (1, 1, 0, 0), all zero, and zz == 0 beside ARBITRARY x, y, zzz."""
        PL, Fo = self.PL(F), self.PL(F).G.F
        return [[Fo.one, Fo.one, Fo.zero, Fo.zero], [Fo.zero] * 4, [PL.rand_elt(rng), PL.rand_elt(rng), Fo.zero, PL.rand_elt(rng)],
                [PL.elt([F.p - 1] * self.g), Fo.zero, Fo.zero, Fo.one]]

    def zs(self, F, rng, n):
        """Z values: 1, p - 1, and random ones (never 0)."""
        PL, Fo = self.PL(F), self.PL(F).G.F
        return [Fo.one, PL.elt([F.p - 1] + [0] * (self.g - 1)), PL.elt([F.p - 1] * self.g)] + [PL.rand_elt(rng) for _ in range(n)]

    def points(self, F, rng, n=28):
        """The patterned points of the layer, the curve points with x in {0, 1, p - 1} (and u, 1 + u over Fq2) that exist — they
        need not lie in the prime-order subgroup, the formulas do not know it — and a chain of sums for variety."""
        PL, G, Fo = self.PL(F), self.PL(F).G, self.PL(F).G.F
        pts = PL.affine_points(rng, nrand=2)
        xs = [Fo.zero, Fo.one, Fo.neg(Fo.one)] + ([(0, 1), (1, 1), (0, F.p - 1)] if self.g == 2 else [])
        special = [P for P in (PL.point_from_x(x) for x in xs) if P is not None]
        assert all(G.on_curve(P) for P in special)
        Q = pts[1]
        chain = []
        while len(chain) < n:
            Q = G.add(Q, pts[2])
            chain.append(Q)
        return special + [G.neg(P) for P in special] + pts + chain, len(special)

    def cases(self, F, rng):
        PL, G, Fo = self.PL(F), self.PL(F).G, self.PL(F).G.F
        pts, nspecial = self.points(F, rng)
        ids = self.identities(F, rng)
        b = self.base
        out = []

        def put(kind, words, want, extra=None):
            out.append((words, None, (kind, want, extra)))

        def other(i):                                       # a point with another x
            Q = pts[(7 * i + 3) % len(pts)]
            return Q if Q[0] != pts[i][0] else G.add(Q, PL.G.gen)
        if b == "dbl_affine":
            for P in pts:
                put("generic", self.enc(F, *P), G.add(P, P))
            for P in pts[:8]:
                put("y = 0", self.enc(F, P[0], Fo.zero), None)
            put("identity", self.enc(F, Fo.zero, Fo.zero), None)
            for _ in range(120):
                P = G.add(pts[rng.randrange(len(pts))], pts[rng.randrange(len(pts))])
                if P is not None:
                    put("generic", self.enc(F, *P), G.add(P, P))
        elif b == "dbl":
            for i, P in enumerate(pts):
                for z in self.zs(F, rng, 3):
                    put("generic", self.enc(F, *self.xyzz(F, P, z)), G.add(P, P))
            for P in pts[:8]:
                c = self.xyzz(F, P, PL.rand_elt(rng))
                put("y = 0", self.enc(F, c[0], Fo.zero, c[2], c[3]), None)
            for I in ids:
                put("identity", self.enc(F, *I), None)
        elif b in ("madd", "madd_fast"):
            fast = b == "madd_fast"
            for i, P in enumerate(pts):
                Q = other(i)
                for z in self.zs(F, rng, 2):
                    a = self.enc(F, *self.xyzz(F, P, z))
                    put("generic", a + self.enc(F, *Q), G.add(P, Q), (True, a))
                    put("addend identity", a + self.enc(F, Fo.zero, Fo.zero), P, (True, a))
                    # P + P with the accumulator under another Z: xyzz_dbl_affine_slow; madd_fast declines
                    put("P + P", a + self.enc(F, *P), G.add(P, P), (not fast, a))
                    put("P + (-P)", a + self.enc(F, *G.neg(P)), None, (not fast, a))
                for I in ids[:3]:
                    a = self.enc(F, *I)
                    put("acc identity", a + self.enc(F, *P), P, (True, a))
            for I in ids:
                a = self.enc(F, *I)
                put("identity + identity", a + self.enc(F, Fo.zero, Fo.zero), None, (True, a))
        elif b == "add":
            for i, P in enumerate(pts):
                Q = other(i)
                zs = self.zs(F, rng, 3)
                for t, z in enumerate(zs):
                    a = self.enc(F, *self.xyzz(F, P, z))
                    z2 = zs[(t + 1) % len(zs)] if t else PL.rand_elt(rng)
                    put("generic", a + self.enc(F, *self.xyzz(F, Q, z2)), G.add(P, Q))
                    # the same point under two different Z: xyzz_dbl_slow
                    put("P + P other Z", a + self.enc(F, *self.xyzz(F, P, PL.rand_elt(rng))), G.add(P, P))
                    put("P + (-P) other Z", a + self.enc(F, *self.xyzz(F, G.neg(P), PL.rand_elt(rng))), None)
                    I = ids[(i + t) % len(ids)]
                    put("addend identity", a + self.enc(F, *I), P)
                    put("acc identity", self.enc(F, *I) + a, P)
                z = PL.rand_elt(rng)
                a = self.enc(F, *self.xyzz(F, P, z))
                put("P + P same Z", a + a, G.add(P, P))
                put("P + (-P) same Z", a + self.enc(F, *self.xyzz(F, G.neg(P), z)), None)
            for I in ids:
                for J in ids:
                    put("identity + identity", self.enc(F, *I) + self.enc(F, *J), None)
        elif b in ("to_affine", "store_jacobian"):
            for P in pts:
                for z in self.zs(F, rng, 4):
                    put("generic", self.enc(F, *self.xyzz(F, P, z)), P)
            for I in ids:
                put("identity", self.enc(F, *I), None)
        else:
            assert b == "from_jacobian"
            for P in pts:
                for z in self.zs(F, rng, 4):
                    put("generic", self.enc(F, Fo.mul(P[0], Fo.sqr(z)), Fo.mul(P[1], Fo.mul(Fo.sqr(z), z)), z), P)
            for X, Y in ((Fo.zero, Fo.one), (Fo.one, Fo.one), (Fo.zero, Fo.zero), (PL.rand_elt(rng), PL.rand_elt(rng))):
                put("identity", self.enc(F, X, Y, Fo.zero), None)
        return out

    def pre(self, F, ctx):
        assert ctx[1] is None or self.PL(F).G.on_curve(ctx[1])

    def check_xyzz(self, F, row, want, tag):
        Fo = self.PL(F).G.F
        x, y, zz, zzz = self.dec(F, row, 4, tag)
        if want is None:
            assert Fo.is_zero(zz), f"{tag}: identity expected (zz == 0), got zz = {zz}"
            return
        assert not Fo.is_zero(zz), f"{tag}: the identity instead of {want}"
        assert Fo.mul(Fo.sqr(zz), zz) == Fo.sqr(zzz), f"{tag}: zz^3 != zzz^2"
        got = (Fo.mul(x, Fo.inv(zz)), Fo.mul(y, Fo.inv(zzz)))
        assert got == want, f"{tag}: point is {got}, want {want}"

    def check(self, F, ctx, row):
        PL, Fo, W = self.PL(F), self.PL(F).G.F, self.W(F)
        kind, want, extra = ctx
        row = [int(v) for v in row]
        tag = f"{self.kind} [{kind}]"
        b = self.base
        if b == "to_affine":
            exp = self.enc(F, *want) if want is not None else [0] * (2 * W)           # the identity is the words (0, 0)
            assert row[:2 * W] == exp, f"{tag}: got {self.dec(F, row, 2, tag)}, want {want}"
        elif b == "store_jacobian":
            X, Y, Z = self.dec(F, row, 3, tag)
            if want is None:
                assert (X, Y, Z) == (Fo.zero, Fo.one, Fo.zero), f"{tag}: the identity is (0, 1, 0), got {(X, Y, Z)}"
                return
            assert not Fo.is_zero(Z), f"{tag}: Z == 0 for {want}"
            z2 = Fo.sqr(Z)
            z6 = Fo.mul(Fo.sqr(z2), z2)
            assert Fo.sqr(Y) == Fo.add(Fo.mul(Fo.sqr(X), X), Fo.mul(PL.G.b, z6)), f"{tag}: Y^2 != X^3 + b Z^6"
            zi = Fo.inv(Z)
            got = (Fo.mul(X, Fo.sqr(zi)), Fo.mul(Y, Fo.mul(Fo.sqr(zi), zi)))
            assert got == want, f"{tag}: point is {got}, want {want}"
        elif b == "madd_fast":
            ret_want, acc = extra
            assert row[4 * W] == int(ret_want), f"{tag}: returned {row[4 * W]}, want {int(ret_want)}"
            if not ret_want:
                assert row[:4 * W] == acc, f"{tag}: returned false but changed the accumulator"
            else:
                self.check_xyzz(F, row, want, tag)
        else:
            self.check_xyzz(F, row, want, tag)


# ------------------------------------------------------------------------------------------------------------ registry
OPS = {}
for _k in ("fp_add", "fp_sub", "fp_neg", "fp_dbl", "fp_mul", "fp_sqr", "fp_reduce_once", "fp_to_mont", "fp_from_mont", "fp_inv", "fp_pow_u64"):
    OPS[_k] = FpOp(_k)
for _k in ("fp2_mul", "fp2_sqr", "fp2_inv"):
    OPS[_k] = FpOp(_k, BASE_FIELDS)
for _k in ("fu_mul", "fu_sqr", "fu_mul_add", "fu_mul_add4"):
    OPS[_k] = FuProduct(_k)
for _k in FuLinear.CFG:
    OPS[_k] = FuLinear(_k)
for _k in ("fu_from_words", "fu_from_sat", "fu_from_sat_reduced", "fu_to_words", "fu_to_sat", "fu_one", "fu_ntt_mul"):
    OPS[_k] = FuConv(_k)
OPS["fu_is_zero_mod_p<2>"] = FuPred("fu_is_zero_mod_p<2>", 2)
OPS["fu_is_multiple_of_p<4>"] = FuPred("fu_is_multiple_of_p<4>", 4)
OPS["fu_maybe_multiple_of_p<4>"] = FuPred("fu_maybe_multiple_of_p<4>", 4)
OPS["xyzz_madd_u"] = MaddOp("xyzz_madd_u", 1)
OPS["xyzz_madd_u2"] = MaddOp("xyzz_madd_u2", 2)
OPS["bk_from_sat"] = BkConvOp("bk_from_sat", 1)
OPS["bk_to_sat"] = BkConvOp("bk_to_sat", 1)
OPS["bk_add"] = BkAddOp("bk_add", 1)
OPS["bk_dbl"] = BkDblOp("bk_dbl", 1)
OPS["bk_add_mem"] = BkAddMemOp("bk_add_mem", 1)
OPS["bk_dbl_mem"] = BkDblMemOp("bk_dbl_mem", 1)
OPS["bk2_from_sat"] = BkConvOp("bk2_from_sat", 2)
OPS["bk2_to_sat"] = BkConvOp("bk2_to_sat", 2)
OPS["bk2_add"] = BkAddOp("bk2_add", 2)
OPS["bk2_dbl"] = BkDblOp("bk2_dbl", 2)
OPS["bk2_add_mem"] = BkAddMemOp("bk2_add_mem", 2)
OPS["bk2_dbl_mem"] = BkDblMemOp("bk2_dbl_mem", 2, identity=False)        # "a is not the identity" (bucket_dev.hpp)
# quad-cooperative forms: the same cases as the single-lane forms they must equal limb for limb
QUAD_OF = {"quad_add_mem": "bk_add_mem", "quad_dbl_mem": "bk_dbl_mem", "quad_add_mem2": "bk2_add_mem"}
OPS["quad_add_mem"] = BkAddMemOp("quad_add_mem", 1)
OPS["quad_dbl_mem"] = BkDblMemOp("quad_dbl_mem", 1)
OPS["quad_add_mem2"] = BkAddMemOp("quad_add_mem2", 2, ["Bn254Fq"])
for _k in EcOp.KINDS:                                       # saturated XYZZ<Fp<P>> / XYZZ<Fp2<P>> (ec_dev.hpp)
    OPS["ec_" + _k] = EcOp("ec_" + _k, 1)
    OPS["ec2_" + _k] = EcOp("ec2_" + _k, 2)

LAYER_OF = {}
for _k in OPS:
    LAYER_OF[_k] = ("fp" if _k.startswith("fp") else "ec" if _k.startswith("ec") else "fu" if _k.startswith("fu_") else "accumulate" if _k.startswith("xyzz") else
                    "quad" if _k.startswith("quad") else "bucket")


def op_seed(op: str, field: str) -> int:
    return SEED ^ (sum(ord(c) * (i + 1) for i, c in enumerate(op + "/" + field)) << 8)


def make_cases(op: str, field: str):
    """Deterministic cases of (op, field): (list of in rows, list of out-init rows or None, list of ctx)."""
    spec, F = OPS[op], FIELDS[field]
    seed_name = QUAD_OF.get(op, op)                        # a quad form gets exactly the cases of its single-lane form
    cases = spec.cases(F, random.Random(op_seed(seed_name, field)))
    return cases


def header_text() -> str:
    return (Path(__file__).resolve().parent.parent / "ckb_zkp_amd" / "csrc" / "unsat_dev.hpp").read_text()
