"""The reference of the device arithmetic probe checks itself (no GPU): tests/field_ref.py against a limb-by-limb model, the
generated operands against the preconditions of the operations they are generated for, and the probe's cross-compile."""
import random

import pytest

from tests import field_ref as R

PRODUCTS = ("fu_mul", "fu_sqr", "fu_mul_add", "fu_mul_add4")


def test_config_matches_header():
    """UNSAT_CFG is a copy of UnsatCfg<P>: L, B, MULCAP, CAPK as unsat_dev.hpp states them."""
    assert R.parse_unsat_cfg(R.header_text()) == R.UNSAT_CFG


def test_mulcap_below_radix_over_modulus():
    """A sum of products with sum KK <= MULCAP stays below 2p iff MULCAP <= floor(R'/p); K p fits the limbs up to CAPK."""
    floors = {n: F.RP // F.p for n, F in R.FIELDS.items()}
    assert floors == {"Bn254Fq": 169, "Bn254Fr": 169, "Bls381Fq": 2520, "Bls381Fr": 70}
    for n, F in R.FIELDS.items():
        assert F.MULCAP <= floors[n]
        assert (F.CAPK + 1) * F.p < (1 << (F.TOPSH + 32)), "CAPK p plus one more addition must fit the limbs"
        assert F.KIN <= F.MULCAP, "from_sat(X) times a value below p"
        assert F.lz(R.KMAX_TABLE)[-1] < (1 << 32)


@pytest.mark.parametrize("field", R.ALL_FIELDS)
def test_closed_form_equals_limb_model(field):
    """(s + m p) / R' is what the product scan returns, limb for limb, on random mul_add calls with operands up to their bounds."""
    F = R.FIELDS[field]
    rng = random.Random(1)
    for _ in range(200):
        ks = [rng.choice((1, 2, 4, 8)) for _ in range(4)]
        ops = [F.limbs(rng.randrange(k * F.p)) for k in ks]
        limbs, worst = F.scan([(ops[0], ops[1]), (ops[2], ops[3])])
        assert worst < (1 << 64)
        assert F.val(limbs) == F.mont([(F.val(ops[0]), F.val(ops[1])), (F.val(ops[2]), F.val(ops[3]))])
        assert F.normalised(limbs)


@pytest.mark.parametrize("op,field", [(op, f) for op in sorted(R.OPS) for f in R.OPS[op].fields])
def test_generated_operands_meet_preconditions(op, field):
    """Value bounds, limb bounds, sum KK <= MULCAP, b < M p, ...: a device mismatch must be the device's fault."""
    spec, F = R.OPS[op], R.FIELDS[field]
    cases = R.make_cases(op, field)
    assert len(cases) >= (1 if op == "fu_one" else 100)
    for words, init, ctx in cases:
        assert all(0 <= int(w) < (1 << 32) for w in words)
        assert init is None or len(init) == spec.nout(F)
        spec.pre(F, ctx)


@pytest.mark.parametrize("field", R.ALL_FIELDS)
@pytest.mark.parametrize("op", PRODUCTS)
def test_column_sums_and_checker(op, field):
    """Over the generated product inputs the model's 64-bit column accumulator never overflows, and the checker accepts the
    model's result and rejects a result that is off by one unit in any one limb, or by p."""
    spec, F = R.OPS[op], R.FIELDS[field]
    cases = R.make_cases(op, field)
    rng = random.Random(2)
    worst_all = 0
    for n, (words, init, ctx) in enumerate(cases):
        limbs, worst = F.scan(spec.prods(F, ctx))
        worst_all = max(worst_all, worst)
        assert worst < (1 << 64), f"{op} {ctx[0]}: column sum {worst / 2 ** 64:.3f} of 2^64"
        spec.check(F, ctx, limbs)
        if n % 16 == 0:
            bad = list(limbs)
            i = rng.randrange(F.L)
            bad[i] ^= 1
            with pytest.raises(AssertionError):
                spec.check(F, ctx, bad)
            with pytest.raises(AssertionError):
                spec.check(F, ctx, F.limbs(F.val(limbs) + F.p))
    print(f"{op} {field}: {len(cases)} cases, worst column sum {worst_all / 2 ** 64:.3f} of 2^64")


def test_mul_add4_with_two_sub_lazy_factors_would_overflow():
    """The margin is real: with limbs at the bound sub_lazy states (2^B + 2^(B+1) - 1), two lazy factors in a sum of four products
    overflow the accumulator of the 9 x 29-bit fields, one does not (unsat_dev.hpp allows one)."""
    for name in ("Bn254Fq", "Bn254Fr", "Bls381Fr"):
        F = R.FIELDS[name]
        full = [F.MASK] * (F.L - 1) + [(2 * F.p) >> F.TOPSH]
        lazy = [(1 << F.B) + (1 << (F.B + 1)) - 1] * (F.L - 1) + [(11 * F.p) >> F.TOPSH]
        _, worst = F.scan([(full, lazy), (full, lazy), (full, full), (full, full)])
        assert worst >= (1 << 64)
        _, worst = F.scan([(full, lazy), (full, full), (full, full), (full, full)])
        assert worst < (1 << 64)
        _, worst = F.scan([(full, lazy), (full, lazy)])     # mul_add with two sub_lazy factors
        assert worst < (1 << 64)


@pytest.mark.parametrize("field", R.ALL_FIELDS)
def test_linear_checker_against_limb_model(field):
    """The checkers of add / sub / csub / sub_lazy accept a Python limb model of the header's loops and reject a dropped carry."""
    F = R.FIELDS[field]

    def carry_chain(terms):                                 # sum of signed limb vectors, normalised like the device's loops
        out, carry = [], 0
        for i in range(F.L):
            t = sum(v[i] for v in terms) + carry
            if i < F.L - 1:
                out.append(t & F.MASK)
                carry = t >> F.B
            else:
                out.append(t & 0xFFFFFFFF)
        return out
    for op in ("fu_add", "fu_sub<2>", "fu_sub<8>", "fu_sub_sub2<6>", "fu_csub<4>", "fu_sub_lazy<9>", "fu_neg_lazy<3>"):
        spec = R.OPS[op]
        for words, init, ctx in R.make_cases(op, field)[::7]:
            cfg, t, m = ctx
            l = [F.limbs(v) for v in t]
            neg = lambda v: [-x for x in v]
            if op == "fu_add":
                r = carry_chain(l)
            elif spec.base == "fu_sub":
                r = carry_chain([l[0], F.mp(spec.M), neg(l[1])])
            elif spec.base == "fu_sub_sub2":
                r = carry_chain([l[0], F.mp(spec.M), neg(l[1]), neg(l[2]), neg(l[2])])
            elif spec.base == "fu_csub":
                r = carry_chain([l[0], neg(F.mp(spec.M))])
                r = l[0] if r[-1] >> 31 else r
            elif spec.base == "fu_sub_lazy":
                r = F.sub_lazy(spec.M, l[0], l[1])
            else:
                r = F.sub_lazy(spec.M, [0] * F.L, l[0])
            spec.check(F, ctx, r)
            bad = list(r)
            bad[1] = (bad[1] + 1) & 0xFFFFFFFF
            with pytest.raises(AssertionError):
                spec.check(F, ctx, bad)


@pytest.mark.parametrize("g", (1, 2))
@pytest.mark.parametrize("field", R.BASE_FIELDS)
def test_point_layer_round_trip(field, g):
    """Accumulators built from an affine point decode to that point at every lift; the searched points are on the curve and
    their Montgomery-form x sits at the pattern."""
    PL = R.layer(field, g)
    rng = random.Random(4)
    pts = PL.affine_points(rng, nrand=2)
    for P in pts:
        assert PL.G.on_curve(P)
        for mode in ("low", "top", "rand"):
            c = PL.acc_coords(P, PL.rand_elt(rng), mode, rng)
            for coord, K in zip(c, PL.BOUNDS):
                assert all((K - 1) * PL.F.p <= v < K * PL.F.p for v in coord) or mode != "top"
            row = PL.point_words(c)
            PL.check_point(row, P, "round trip")
            with pytest.raises(AssertionError):
                PL.check_point(row, PL.G.add(P, P), "round trip")
    P = pts[0]
    c = PL.acc_coords(P, PL.rand_elt(rng), "low", rng)
    c[0] = tuple(v + PL.KX * PL.F.p for v in c[0])          # right mod p, above its stored bound: must be rejected
    with pytest.raises(AssertionError):
        PL.check_point(PL.point_words(c), P, "bound")


def test_probe_cross_compiles():
    """The probe builds for gfx950 against the unchanged product headers, and exports its one entry."""
    import ctypes

    from tests import field_probe
    lib = field_probe.build()
    assert lib.exists()
    assert hasattr(ctypes.CDLL(str(lib)), "zkp_probe_run")


def _ec_model(spec, F, words):
    """The formulas of ec_dev.hpp (dbl-2008-s-1, madd-2008-s, add-2008-s, a = 0) over oracle/pyref field elements: the words a
    correct device returns for the input row `words`."""
    Fo, W, b = spec.PL(F).G.F, spec.W(F), spec.base
    inf = [Fo.one, Fo.one, Fo.zero, Fo.zero]
    sub, mul, sqr, dbl_ = Fo.sub, Fo.mul, Fo.sqr, lambda a: Fo.small(a, 2)

    def dbl(p, aff=False):
        x, y = p[0], p[1]
        if (aff and Fo.is_zero(x) and Fo.is_zero(y)) or (not aff and Fo.is_zero(p[2])) or Fo.is_zero(y):
            return inf
        u = dbl_(y)
        v = sqr(u)
        w = mul(u, v)
        s = mul(x, v)
        m = Fo.small(sqr(x), 3)
        x3 = sub(sqr(m), dbl_(s))
        y3 = sub(mul(m, sub(s, x3)), mul(w, y))
        return [x3, y3, v, w] if aff else [x3, y3, mul(v, p[2]), mul(w, p[3])]

    def add(p, o, fast=False):
        """o: XYZZ; an affine addend comes as (x, y, 1, 1) or, for the identity, with zz = 0."""
        if Fo.is_zero(o[2]):
            return p, True
        if Fo.is_zero(p[2]):
            return list(o), True
        u1, u2, s1, s2 = mul(p[0], o[2]), mul(o[0], p[2]), mul(p[1], o[3]), mul(o[1], p[3])
        pp_, r = sub(u2, u1), sub(s2, s1)
        if Fo.is_zero(pp_):
            if fast:
                return p, False
            return (dbl(p) if Fo.is_zero(r) else inf), True
        pp = sqr(pp_)
        ppp = mul(pp_, pp)
        q = mul(u1, pp)
        x3 = sub(sub(sqr(r), ppp), dbl_(q))
        y3 = sub(mul(r, sub(q, x3)), mul(s1, ppp))
        return [x3, y3, mul(mul(p[2], o[2]), pp), mul(mul(p[3], o[3]), ppp)], True
    n_in = {"dbl_affine": 2, "dbl": 4, "madd": 6, "madd_fast": 6, "add": 8, "to_affine": 4, "store_jacobian": 4, "from_jacobian": 3}[b]
    c = spec.dec(F, words, n_in, "model input")
    if b == "dbl_affine":
        return spec.enc(F, *dbl(c, aff=True))
    if b == "dbl":
        return spec.enc(F, *dbl(c))
    if b in ("madd", "madd_fast"):
        o = [c[4], c[5]] + ([Fo.zero, Fo.zero] if Fo.is_zero(c[4]) and Fo.is_zero(c[5]) else [Fo.one, Fo.one])
        res, ret = add(c[:4], o, fast=b == "madd_fast")
        return spec.enc(F, *res) + ([int(ret)] if b == "madd_fast" else [])
    if b == "add":
        return spec.enc(F, *add(c[:4], c[4:])[0])
    if b == "to_affine":
        if Fo.is_zero(c[2]):
            return spec.enc(F, Fo.zero, Fo.zero)
        return spec.enc(F, mul(c[0], Fo.inv(c[2])), mul(c[1], Fo.inv(c[3])))
    if b == "store_jacobian":
        if Fo.is_zero(c[2]):
            return spec.enc(F, Fo.zero, Fo.one, Fo.zero)
        t = mul(c[2], sqr(c[3]))
        return spec.enc(F, mul(c[0], t), mul(mul(c[1], t), sqr(c[2])), mul(c[2], c[3]))
    if Fo.is_zero(c[2]):
        return spec.enc(F, *inf)
    return spec.enc(F, c[0], c[1], sqr(c[2]), mul(sqr(c[2]), c[2]))


@pytest.mark.parametrize("op,field", [(op, f) for op in sorted(R.OPS) if R.LAYER_OF[op] == "ec" for f in R.OPS[op].fields])
def test_ec_checker_against_formula_model(op, field):
    """The checks of the ec_dev.hpp operations accept what the header's formulas give in Python integers on every generated case
    (so the expected points, built from the affine group law alone, are right) and reject a row with one word changed, the
    negated point, and a non-canonical coordinate."""
    spec, F = R.OPS[op], R.FIELDS[field]
    cases = R.make_cases(op, field)
    kinds = {c[2][0] for c in cases}
    assert {"generic", "identity"} <= kinds or {"generic", "P + P", "P + (-P)", "acc identity", "addend identity", "identity + identity"} <= kinds \
        or {"generic", "P + P other Z", "P + P same Z", "P + (-P) other Z", "acc identity", "addend identity", "identity + identity"} <= kinds
    rng = random.Random(9)
    W = spec.W(F)
    for n, (words, init, ctx) in enumerate(cases):
        assert len(words) == len(cases[0][0])
        row = _ec_model(spec, F, words)
        assert len(row) == spec.nout(F)
        spec.check(F, ctx, row)
        if ctx[1] is None or (spec.base == "madd_fast" and not ctx[2][0]):
            continue
        if n % 8 == 0:
            bad = list(row)
            bad[rng.randrange(len(row) - (spec.base == "madd_fast"))] ^= 1 << rng.randrange(8)
            with pytest.raises(AssertionError):
                spec.check(F, ctx, bad)
            bad = list(row)                                 # -P: y -> p - y in the first component
            y = F.from_words(row[W:W + F.N])
            if y:
                bad[W:W + F.N] = F.words(F.p - y)
                with pytest.raises(AssertionError):
                    spec.check(F, ctx, bad)
            bad = list(row)                                 # x + p: right mod p, not canonical
            x = F.from_words(row[:F.N]) + F.p
            if x < F.R:
                bad[:F.N] = F.words(x)
                with pytest.raises(AssertionError):
                    spec.check(F, ctx, bad)
