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
