"""CPU: the pairing's codecs, constants and formulas, without a device.

* fq12_from_mont / fq12_to_mont are inverse to each other, and the tower <-> flat index map they embody is a ring isomorphism (a
  tower product written out in Python against oracle.pyref.pairing.Fp12.mul);
* every word of csrc/pairing_constants.inc equals its definition recomputed here in Python integers, and the committed file is what
  tools/gen_pairing_constants.py prints;
* E = e(G1, G2) of the oracle has order r and is not 1;
* the model of the device's formulas (tests/pairing_ref.py: projective Miller loop, Granger-Scott squaring, the hard-part chains)
  agrees with the oracle through bilinearity, and csrc/pairing_dev.hpp itself, instantiated with a plain C++ field
  (tests/c/pairing_host.cpp), agrees with that model word for word, the raw Miller value included."""
import os
import random
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from ckb_zkp_amd import codec
from ckb_zkp_amd import pairing as zp
from ckb_zkp_amd.params import get_curve
from oracle.pyref.fields import f2_inv, f2_mul
from oracle.pyref.pairing import Fp12
from tests import pairing_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
INC = CSRC / "pairing_constants.inc"
STRUCT = {"bn254": "Bn254Pairing", "bls12_381": "Bls381Pairing"}
CURVES = list(ref.CURVE_NAMES)


def _random_flat(c, rng):
    return [(rng.randrange(c.q), rng.randrange(c.q)) for _ in range(6)]


@pytest.mark.parametrize("curve", CURVES)
def test_codec_round_trip(curve):
    c = get_curve(curve)
    rng = random.Random(f"codec-{curve}")
    for f in [_random_flat(c, rng), zp.gt_one(), [(0, 0)] * 6, [(c.q - 1, c.q - 1)] * 6]:
        w = zp.fq12_to_mont(f, c)
        assert w.shape == (12 * c.fq_limbs,) and w.dtype == np.uint64
        assert zp.fq12_from_mont(w, c) == f
        assert np.array_equal(zp.fq12_to_mont(zp.fq12_from_mont(w, c), c), w)
    # position p of the ABI holds the coefficient of w^TOWER_TO_FLAT[p]
    for pos, k in enumerate(ref.TOWER_TO_FLAT):
        f = [(0, 0)] * 6
        f[k] = (1, 0)
        w = zp.fq12_to_mont(f, c).reshape(12, c.fq_limbs)
        assert [i for i in range(12) if w[i].any()] == [2 * pos]


@pytest.mark.parametrize("curve", CURVES)
def test_tower_and_flat_are_isomorphic(curve):
    c = ref.curve(curve)
    T, F = ref.tower(curve), Fp12(c)
    rng = random.Random(f"iso-{curve}")
    for _ in range(4):
        a, b = T.random(rng), T.random(rng)
        assert T.to_flat(T.mul(a, b)) == F.mul(T.to_flat(a), T.to_flat(b))
        assert T.from_flat(T.to_flat(a)) == a
        assert T.sqr(a) == T.mul(a, a)
        assert T.mul(a, T.inv(a)) == T.one
        for k in (1, 2, 3):
            assert T.to_flat(T.frob(a, k)) == F.pow(T.to_flat(a), c.q ** k)
    assert T.to_flat(T.one) == F.one


def _parse_inc():
    text = INC.read_text()
    out = {}
    for m in re.finditer(r"struct (\w+) \{(.*?)\n\};", text, flags=re.S):
        body, d = m.group(2), {}
        for a in re.finditer(r"static constexpr uint32_t (\w+)((?:\[\d+\])+) = (\{.*?\});", body, flags=re.S):
            d[a.group(1)] = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", a.group(3))]
        for a in re.finditer(r"static constexpr (?:int|bool|uint64_t) (\w+) = (true|false|0x[0-9a-f]+|\d+)", body):
            v = a.group(2)
            d[a.group(1)] = {"true": 1, "false": 0}[v] if v in ("true", "false") else int(v, 0)
        out[m.group(1)] = d
    return out


def _f2_pow(a, e, p):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f2_mul(r, r, p)
        if bit == "1":
            r = f2_mul(r, a, p)
    return r


@pytest.mark.parametrize("curve", CURVES)
def test_every_constant_equals_its_definition(curve):
    c = ref.curve(curve)
    d = _parse_inc()[STRUCT[curve]]
    q, n = c.q, 2 * c.fq_limbs
    R = 1 << (32 * n)

    def fq(words):
        assert len(words) == n
        v = sum(w << (32 * i) for i, w in enumerate(words))
        assert v < q, "not reduced"
        return v * pow(R, -1, q) % q

    def fq2s(words):
        assert len(words) % (2 * n) == 0
        return [(fq(words[k:k + n]), fq(words[k + n:k + 2 * n])) for k in range(0, len(words), 2 * n)]

    bn = curve == "bn254"
    x = c.x_param if bn else -c.x_param
    loop = 6 * x + 2 if bn else c.x_param
    assert d["BN"] == (1 if bn else 0) and d["TWIST_D"] == (1 if c.twist_is_d else 0)
    assert (d["XI0"], 1) == c.xi
    assert d["ABS_X"] == c.x_param and d["X_NEG"] == (0 if bn else 1)
    assert d["LOOP_BITS"] == loop.bit_length() and sum(w << (32 * i) for i, w in enumerate(d["LOOP"])) == loop
    assert fq(d["TWO_INV"]) * 2 % q == 1
    (tb,) = fq2s(d["TWIST_B"])
    assert tb == c.g2_b == (f2_mul((c.g1_b, 0), f2_inv(c.xi, q), q) if c.twist_is_d else f2_mul((c.g1_b, 0), c.xi, q))
    frob = fq2s(d["FROB"])
    assert len(frob) == 18
    for k in (1, 2, 3):
        for j in range(6):
            assert frob[6 * (k - 1) + j] == _f2_pow(c.xi, j * (q ** k - 1) // 6, q), (k, j)
    if bn:
        assert fq2s(d["TWIST_FROB_X"]) == [_f2_pow(c.xi, (q - 1) // 3, q)]
        assert fq2s(d["TWIST_FROB_Y"]) == [_f2_pow(c.xi, (q - 1) // 2, q)]
    else:
        assert "TWIST_FROB_X" not in d and "TWIST_FROB_Y" not in d
    # the contract's power: the chain's exponent, as a polynomial in q, is k times the hard part
    h = (q ** 4 - q ** 2 + 1) // c.r
    if bn:
        e = q ** 3 + (6 * x * x + 1) * q ** 2 + (-36 * x ** 3 - 18 * x * x - 12 * x + 1) * q + (-36 * x ** 3 - 30 * x * x - 18 * x - 2)
    else:
        e = (x - 1) ** 2 * (x + q) * (x * x + q * q - 1) + 3
    assert e == d["GT_POWER"] * h
    assert d["GT_POWER"] == zp.GT_POWER[curve] == ref.GT_POWER[curve] and d["GT_POWER"] % c.r != 0


def test_the_committed_constants_are_the_generators_output():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_pairing_constants.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == INC.read_text()


@pytest.mark.parametrize("curve", CURVES)
def test_generator_pairing_has_order_r(curve):
    c = ref.curve(curve)
    F = Fp12(c)
    E = list(ref.gen_pairing(curve))
    assert E != F.one
    assert F.pow(E, c.r) == F.one                            # r is prime: the order is r


@pytest.mark.parametrize("curve", CURVES)
def test_model_agrees_with_the_oracle(curve):
    c = ref.curve(curve)
    T, F = ref.tower(curve), Fp12(c)
    rng = random.Random(f"model-{curve}")
    a = T.random(rng)
    assert T.to_flat(T.final_exp(a)) == F.pow(T.to_flat(a), ref.GT_POWER[curve] * ((c.q ** 12 - 1) // c.r))   # one oracle power
    g = T.final_exp(a)
    assert T.cyclotomic_sqr(g) == T.sqr(g)
    for x, y in [(1, 1), (2, 3), (c.r - 1, 1), (rng.randrange(c.r), rng.randrange(c.r))]:
        f = T.miller(ref.g1_mul(curve, x), ref.g2_mul(curve, y))
        assert T.to_flat(T.final_exp(f)) == ref.expected_pairing(curve, x, y), (x, y)
    assert T.miller(None, c.g2_gen) == T.one and T.miller(c.g1_gen, None) == T.one


@pytest.fixture(scope="module")
def host_program():
    out = ROOT / "tests" / "c" / "build" / "pairing_host"
    out.parent.mkdir(parents=True, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", f"-I{CSRC}", str(ROOT / "tests" / "c" / "pairing_host.cpp"), "-o",
           str(out)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_the_device_header_on_a_cpu_field(curve, host_program):
    c = get_curve(curve)
    T = ref.tower(curve)
    rng = random.Random(f"host-{curve}")

    def words(a):
        return " ".join("%08x" % x for x in np.ascontiguousarray(a).view("<u4").ravel())

    def parse(line):
        return zp.fq12_from_mont(np.array([int(x, 16) for x in line.split()], dtype="<u4").view("<u8"), c)

    reqs, want = [], []
    for a, b in [(1, 1), (c.r - 1, 2), (rng.randrange(c.r), rng.randrange(c.r))]:
        P, Q = ref.g1_mul(curve, a), ref.g2_mul(curve, b)
        pts = words(codec.g1_to_mont([P], c)[0]) + " " + words(codec.g2_to_mont([Q], c)[0])
        reqs += ["P " + pts, "M " + pts]
        want += [ref.expected_pairing(curve, a, b), T.to_flat(T.miller(P, Q))]
    x, y = T.random(rng), T.random(rng)
    fx, fy = T.to_flat(x), T.to_flat(y)
    reqs += ["F " + words(zp.fq12_to_mont(fx, c)), "X " + words(zp.fq12_to_mont(fx, c)) + " " + words(zp.fq12_to_mont(fy, c)),
             "F " + words(zp.fq12_to_mont([(0, 0)] * 6, c)), "F " + words(zp.fq12_to_mont(zp.gt_one(), c))]
    want += [T.to_flat(T.final_exp(x)), T.to_flat(T.mul(x, y)), [(0, 0)] * 6, zp.gt_one()]
    reqs.append("C " + pts)                                              # the product counts that tools/pairing_bench.py reports against
    r = subprocess.run([str(host_program), str(c.cid)], input="\n".join(reqs) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert [int(x) for x in lines.pop().split()] == [zp.FQ_PRODUCTS[curve]["miller"], zp.FQ_PRODUCTS[curve]["final_exp"]]
    reqs.pop()
    assert len(lines) == len(want)
    for req, line, w in zip(reqs, lines, want):
        assert parse(line) == w, req[:1]
