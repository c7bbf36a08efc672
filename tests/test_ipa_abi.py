"""CPU: the IPA generator fold (zkp_g1_ipa_fold_dev) and the batched Fr inner products (zkp_fr_dot_batch_dev) are exported,
declared, bound in Python, and reject a NULL context or NULL arrays without touching a device."""
import ctypes
import re
from pathlib import Path

from ckb_zkp_amd import _lib, ipa
from ckb_zkp_amd.api import Context

ROOT = Path(__file__).resolve().parent.parent
SYMS = ("zkp_g1_ipa_fold_dev", "zkp_fr_dot_batch_dev")


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s


def test_version():
    assert _lib.load().zkp_version().startswith(b"zkp_accel 0.7.1")


def test_header_declares():
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    for s in SYMS:
        assert re.search(r"int32_t\s+" + s + r"\s*\(", text), s


def test_python_surface():
    for m in ("ipa_fold_dev", "ipa_fold", "fr_dot_batch_dev"):
        assert callable(getattr(Context, m, None)), m
    assert callable(ipa.inner_product_prove)


def test_null_context_and_arrays_are_bad_arg():
    lib = _lib.load()
    k = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    buf = (ctypes.c_uint64 * 64)()
    flags = (ctypes.c_uint8 * 8)()
    fold = lib.zkp_g1_ipa_fold_dev
    assert fold(None, 0, None, None, None, None, 0, None, None, None, None) == -1          # n == 0, NULL context
    assert fold(None, 0, buf, None, buf, None, 4, k, k, buf, flags) == -1
    assert fold(None, 0, None, None, None, None, 4, None, None, None, None) == -1          # n > 0, NULL arrays
    dot = lib.zkp_fr_dot_batch_dev
    ns = (ctypes.c_size_t * 1)(4)
    ptrs = (ctypes.c_void_p * 1)(None)
    out = (ctypes.c_uint64 * 4)()
    assert dot(None, 0, 0, None, None, None, None) == -1
    assert dot(None, 0, 1, ptrs, ptrs, ns, out) == -1
    assert dot(None, 0, 1, None, None, None, out) == -1
