"""CPU: the fused sum-check round (zkp_fr_sumcheck_round_dev) and the eq table (zkp_fr_eq_evals_dev) are exported, declared, bound
in Python, and reject a NULL context or NULL arrays without touching a device."""
import ctypes
import re
from pathlib import Path

from ckb_zkp_amd import _lib, api, sumcheck
from ckb_zkp_amd.api import Context

ROOT = Path(__file__).resolve().parent.parent
SYMS = ("zkp_fr_sumcheck_round_dev", "zkp_fr_eq_evals_dev")


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s


def test_header_declares():
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    for s in SYMS:
        assert re.search(r"int32_t\s+" + s + r"\s*\(", text), s
    assert re.search(r"ZKP_SC_EQ_AB_MINUS_C\s*=\s*0\s*,\s*ZKP_SC_PROD2\s*=\s*1\s*,\s*ZKP_SC_PROD3\s*=\s*2", text)
    assert (api.SC_EQ_AB_MINUS_C, api.SC_PROD2, api.SC_PROD3) == (0, 1, 2)


def test_python_surface():
    for m in ("fr_sumcheck_round_dev", "fr_eq_evals_dev", "fr_eq_evals"):
        assert callable(getattr(Context, m, None)), m
    for f in ("prove_phase_one", "prove_phase_two", "prove_cubic_batched", "r1cs_sumcheck"):
        assert callable(getattr(sumcheck, f, None)), f


def test_host_coefficients_match_interpolation():
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    poly = [5, r - 3, 7, 11]                                               # d, c, b, a
    g = lambda x: sum(c * x ** i for i, c in enumerate(poly)) % r          # noqa: E731
    assert sumcheck.cubic_coeffs(g(0), g(2), g(3), (g(0) + g(1)) % r, r) == poly
    quad = [9, 4, r - 1]
    g = lambda x: sum(c * x ** i for i, c in enumerate(quad)) % r          # noqa: E731
    assert sumcheck.quadratic_coeffs(g(0), g(2), (g(0) + g(1)) % r, r) == quad


def test_null_context_and_arrays_are_bad_arg():
    lib = _lib.load()
    x = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    out = (ctypes.c_uint64 * 12)()
    buf = (ctypes.c_uint64 * 64)()
    ptrs = (ctypes.c_void_p * 4)(ctypes.addressof(buf), ctypes.addressof(buf), ctypes.addressof(buf), ctypes.addressof(buf))
    rnd = lib.zkp_fr_sumcheck_round_dev
    assert rnd(None, 0, 0, 1, ptrs, 4, x, out) == -1                       # NULL context
    assert rnd(None, 0, 0, 0, None, 4, None, out) == -1                    # count == 0, NULL context
    assert rnd(None, 0, 0, 1, None, 4, x, out) == -1                       # NULL table array
    assert rnd(None, 0, 0, 1, ptrs, 4, None, None) == -1                   # neither bind nor evaluations
    eq = lib.zkp_fr_eq_evals_dev
    assert eq(None, 0, x, 1, buf) == -1
    assert eq(None, 0, None, 0, buf) == -1
    assert eq(None, 0, None, 1, buf) == -1                                 # k > 0, NULL challenges
    assert eq(None, 0, x, 1, None) == -1                                   # NULL output
