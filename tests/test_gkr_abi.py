"""CPU: the Libra GKR entry points are declared, exported and bound, their constants agree between gkr.hpp and gkr.py, and every
entry rejects a NULL context or NULL arrays without dereferencing anything (no compute calls).  The wiring rules of
zkp_gkr_layer_upload (op, node range, gate count) need a live context and are in tests/test_gpu_gkr.py test_upload_rules."""
import ctypes
import re
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, gkr
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["zkp_gkr_layer_upload", "zkp_gkr_layer_free", "zkp_gkr_layer_info", "zkp_fr_gkr_eval_layer_dev", "zkp_fr_gkr_tables_dev",
         "zkp_fr_gkr_round_dev"]
V = ctypes.c_void_p


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    declared = header_symbols()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    ffi = (ROOT / "rust" / "zkp-accel" / "src" / "ffi.rs").read_text()
    for name in NAMES:
        assert f"pub fn {name}(" in ffi, name
    assert "pub struct zkp_gkr_layer {" in ffi


def test_constants_agree_with_the_header():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "gkr.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (GKR_[A-Z]+) = (\d+);", hpp)}
    assert consts == {"GKR_LONG": gkr.GKR_LONG, "GKR_CHUNK": gkr.GKR_CHUNK}
    assert 2 <= gkr.GKR_LONG < gkr.GKR_CHUNK
    # the public header quotes both numbers in the contract of zkp_gkr_layer_upload
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert f"more than {gkr.GKR_LONG} entries into chunks of {gkr.GKR_CHUNK}" in text


def test_null_context_and_null_arrays_are_rejected():
    lib = _lib.load()
    op = np.array([0, 1], dtype=np.uint8)
    left = np.array([0, 1], dtype=np.uint32)
    right = np.array([1, 0], dtype=np.uint32)
    fr = np.zeros((8, 4), dtype=np.uint64)
    info = (ctypes.c_uint64 * 8)()
    handle = V()
    p = lambda a: V(a.ctypes.data)                                 # noqa: E731
    fake = V(fr.ctypes.data)                                       # a non-NULL stand-in: a NULL context returns before any use
    tabs = (V * 4)(fake, fake, fake, fake)
    # NULL context
    assert lib.zkp_gkr_layer_upload(None, p(op), p(left), p(right), 2, 1, ctypes.byref(handle)) == -1
    assert handle.value is None
    assert lib.zkp_gkr_layer_free(None, fake) == -1
    assert lib.zkp_fr_gkr_eval_layer_dev(None, 0, fake, fake, fake) == -1
    assert lib.zkp_fr_gkr_tables_dev(None, 0, fake, 1, fake, fake, tabs) == -1
    assert lib.zkp_fr_gkr_round_dev(None, 0, 1, tabs, 4, fake, fake, fake) == -1
    # NULL arrays / handles (checked before the context is touched, so a stand-in context is never dereferenced)
    for args in ((None, p(left), p(right)), (p(op), None, p(right)), (p(op), p(left), None)):
        assert lib.zkp_gkr_layer_upload(fake, *args, 2, 1, ctypes.byref(handle)) == -1
    assert lib.zkp_gkr_layer_upload(fake, p(op), p(left), p(right), 2, 1, None) == -1
    assert lib.zkp_gkr_layer_free(fake, None) == -1
    assert lib.zkp_gkr_layer_info(None, info) == -1 and lib.zkp_gkr_layer_info(fake, None) == -1
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.zkp_fr_gkr_eval_layer_dev(fake, 0, *args) == -1
    for args in ((None, 1, fake, fake, tabs), (fake, 1, None, fake, tabs), (fake, 1, fake, None, tabs), (fake, 1, fake, fake, None)):
        assert lib.zkp_fr_gkr_tables_dev(fake, 0, *args) == -1
    assert lib.zkp_fr_gkr_round_dev(fake, 0, 1, None, 4, fake, fake, fake) == -1
    assert lib.zkp_fr_gkr_round_dev(fake, 0, 1, tabs, 4, fake, None, None) == -1
    assert handle.value is None

