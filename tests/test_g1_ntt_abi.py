"""CPU: the G1 transform entry points (zkp_g1_scale_vec_dev / zkp_g1_ntt_dev) are declared, exported, bound and present in the
generated Rust declarations, their constants agree between g1_ntt.hpp, asvc.py and the public header, both entries reject a NULL
context or NULL required pointers without dereferencing anything (no compute calls), and the convolution arrangement of
asvc.prove_all gives the single-position quotients in Python integers.  Every other argument rule needs a live context and is in
tests/test_gpu_g1_ntt.py."""
import ctypes
import random
import re
from pathlib import Path

import numpy as np
import pytest

from ckb_zkp_amd import _lib, asvc
from ckb_zkp_amd.api import Context
from ckb_zkp_amd.params import get_curve
from oracle.pyref.fields import CURVES
from tests import asvc_ref as ref
from tests import g1_ntt_ref
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"zkp_g1_scale_vec_dev": 8, "zkp_g1_ntt_dev": 6}
V = ctypes.c_void_p


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    declared = header_symbols()
    ffi = (ROOT / "rust" / "zkp-accel" / "src" / "ffi.rs").read_text()
    for name, arity in NAMES.items():
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert f"pub fn {name}(" in ffi, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
    assert "ZKP_G1_NTT_MAX_LOG" in ffi
    for method in ("g1_scale_vec_dev", "g1_ntt_dev", "g1_scale_vec", "g1_ntt"):
        assert callable(getattr(Context, method))
    # the version comment lists them among the entries detected by symbol
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert " / ".join(NAMES) in text[:text.index("const char* zkp_version(void);")]


def test_constants_agree():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "g1_ntt.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (G1N_[A-Z_]+) = (\d+);", hpp)}
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    max_log = int(re.search(r"#define ZKP_G1_NTT_MAX_LOG (\d+)", text).group(1))
    assert consts["G1N_MAX_LOG"] == max_log == asvc.G1_NTT_MAX_LOG
    assert consts["G1N_LANES"] == asvc.G1_NTT_LANES == 64
    assert 21 <= max_log <= min(get_curve(c).two_adicity for c in CURVES)
    assert consts["G1N_SCALAR_BITS"] == 256 and all(get_curve(c).r < 1 << 255 for c in CURVES)   # no carry out of the top window


def test_null_context_and_null_pointers_are_rejected():
    lib = _lib.load()
    buf = np.zeros((8, 12), dtype=np.uint64)
    fake = V(buf.ctypes.data)                                        # non-NULL stand-in: a NULL context returns before any use
    assert lib.zkp_g1_scale_vec_dev(None, 0, fake, None, fake, 2, fake, fake) == -1
    assert lib.zkp_g1_ntt_dev(None, 0, fake, fake, 1, 0) == -1
    # NULL required pointers (checked before the context is touched, so a stand-in context is never dereferenced)
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert lib.zkp_g1_scale_vec_dev(fake, 0, args[0], None, args[1], 2, args[2], args[3]) == -1
    assert lib.zkp_g1_ntt_dev(fake, 0, None, fake, 1, 0) == -1
    assert lib.zkp_g1_ntt_dev(fake, 0, fake, None, 1, 0) == -1
    assert (buf == 0).all()


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("curve", list(CURVES))
def test_convolution_arrangement_gives_the_quotients(curve, n):
    """prove_all's steps with the exponent in place of the point: q_i(tau) for every i, against long division"""
    c = CURVES[curve]
    rng = random.Random(f"g1-ntt-conv-{curve}-{n}")
    tau = rng.randrange(2, c.r)
    for values in ([rng.randrange(c.r) for _ in range(n)], [c.r - 1] * n, [rng.randrange(c.r)], [0] * n):
        got = g1_ntt_ref.prove_all_exponents(curve, n, tau, values)
        want = [ref.poly_eval(ref.witness_polynomial(c, n, values, [i]), tau, c.r) for i in range(n)]
        assert got == want, (curve, n)
