"""asvc.all_proofs_key / prove_all / lagrange_from_powers on the device: every proof bit-exact against the long division of
tests/asvc_ref.py in the exponent and against the device's own prove_pos, the aggregate of prove_all's outputs against the subvector
proof, the keyless Lagrange key against key_gen's trapdoor-derived one.  n = 2 is one butterfly per transform of size n, 64 the first
size whose size-2n transforms fill a wave, 256 two and four workgroups."""
import random

import numpy as np
import pytest

from ckb_zkp_amd import asvc, codec
from ckb_zkp_amd.params import get_curve
from tests import asvc_cases as cases
from tests import asvc_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SIZES = [2, 4, 8, 64, 256]


def _mont_g(c):
    oc = cases.inputs(c.name)[0]
    g1, g2 = cases.generators(oc)
    return codec.g1_to_mont([g1], c)[0][0], codec.g2_to_mont([g2], c)[0][0], g1, oc


def _tau(n):
    return cases.TAU + 7 * n


@pytest.fixture(scope="module")
def keys(ctx):
    """(curve, n) -> (uploaded proving key, all-proofs key), made on first use"""
    made = {}

    def get(curve, n):
        if (curve, n) not in made:
            c = get_curve(curve)
            g1m, g2m, _, _ = _mont_g(c)
            pk = asvc.key_gen(ctx, c, n, _tau(n), g1m, g2m).proving_key.upload(ctx)
            made[(curve, n)] = (pk, asvc.all_proofs_key(ctx, pk))
        return made[(curve, n)]

    yield get
    for pk, apk in made.values():
        apk.free()
        pk.free()


def value_sets(c, n, rng):
    one = [0] * n
    one[rng.randrange(n)] = rng.randrange(1, c.r)
    v = rng.randrange(1, c.r)
    return {"random": [rng.randrange(c.r) for _ in range(n)], "zero": [0] * n, "equal": [v] * n, "one_nonzero": one,
            "fewer": [rng.randrange(c.r) for _ in range(max(1, n - 1 - n // 4))], "rmax": [c.r - 1] * n}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_prove_all(ctx, keys, curve, n):
    c = get_curve(curve)
    _, _, g1, oc = _mont_g(c)
    pk, apk = keys(curve, n)
    rng = random.Random(f"asvc-all-{curve}-{n}")
    checked = list(range(n)) if n <= 64 else sorted(rng.sample(range(n), 16))
    on_device = sorted({0, n // 2, n - 1} | set(rng.sample(range(n), min(3, n))))
    for name, values in value_sets(c, n, rng).items():
        xy, inf = asvc.prove_all(pk, apk, values)
        assert xy.shape == (n, 2 * c.fq_limbs) and inf.shape == (n,)
        want = [ref.prove_pos_in_exponent(oc, n, _tau(n), g1, values, [i]) for i in checked]
        want_xy, want_inf = codec.g1_to_mont(want, c)
        assert np.array_equal(xy[checked], want_xy) and np.array_equal(inf[checked], want_inf), (curve, n, name)
        for i in on_device:
            p_xy, p_inf = asvc.prove_pos(pk, values, [i])
            assert np.array_equal(xy[i], p_xy) and bool(inf[i]) == p_inf, (curve, n, name, i)


@pytest.mark.parametrize("curve", CURVES)
def test_aggregate_of_all_proofs(ctx, keys, curve):
    c = get_curve(curve)
    n = 64
    pk, apk = keys(curve, n)
    rng = random.Random(f"asvc-all-agg-{curve}")
    values = [rng.randrange(c.r) for _ in range(n)]
    subset = rng.sample(range(n), 5)
    xy, inf = asvc.prove_all(pk, apk, values)
    got = asvc.aggregate_proofs(ctx, c, n, subset, [(xy[i], bool(inf[i])) for i in subset])
    want = asvc.prove_pos(pk, values, subset)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]


@pytest.mark.parametrize("n", [8, 128])
@pytest.mark.parametrize("curve", CURVES)
def test_lagrange_from_powers(ctx, curve, n):
    c = get_curve(curve)
    g1m, g2m, _, _ = _mont_g(c)
    pk = asvc.key_gen(ctx, c, n, _tau(n), g1m, g2m).proving_key
    xy, inf = asvc.lagrange_from_powers(ctx, c, pk.powers_of_g1, n)
    assert np.array_equal(xy, pk.l_of_g1) and not inf.any()


@pytest.mark.parametrize("curve", CURVES)
def test_keys_and_proofs_repeat(ctx, keys, curve):
    """all_proofs_key built twice is identical; prove_all twice on one key, with another vector in between, returns the same"""
    c = get_curve(curve)
    n = 64
    pk, apk = keys(curve, n)
    again = asvc.all_proofs_key(ctx, pk)
    try:
        w = 2 * c.fq_limbs
        tables = []
        for k in (apk, again):
            xy, inf = np.zeros((2 * n, w), dtype=np.uint64), np.zeros(2 * n, dtype=np.uint8)
            ctx.d2h(xy, k.a_xy)
            ctx.d2h(inf, k.a_inf)
            tables.append((xy, inf))
        assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1])
        assert not tables[0][1].any()
    finally:
        again.free()
    rng = random.Random(f"asvc-all-repeat-{curve}")
    values, other = ([rng.randrange(c.r) for _ in range(n)] for _ in range(2))
    first = asvc.prove_all(pk, apk, values)
    asvc.prove_all(pk, apk, other)
    second = asvc.prove_all(pk, apk, values)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


@pytest.mark.parametrize("curve", CURVES)
def test_prove_all_argument_rules(ctx, keys, curve):
    c = get_curve(curve)
    pk, apk = keys(curve, 8)
    _, other = keys(curve, 4)
    with pytest.raises(ValueError):
        asvc.prove_all(pk, other, [1] * 8)                           # a key of another size
    with pytest.raises(ValueError):
        asvc.prove_all(pk, apk, [1] * 9)
    with pytest.raises(ValueError):
        asvc.prove_all(pk, apk, [])
    with pytest.raises(ValueError):
        asvc._g1_log(c, 1 << asvc.G1_NTT_MAX_LOG + 1)                # 2n beyond the largest G1 transform
