"""CPU: the PLONK entry points are declared, exported and bound, their blocking constants agree between plonk.hpp and plonk.py,
and every entry rejects a NULL context or NULL arrays without dereferencing anything (no compute calls).  The domain, scalar and
aliasing rules need a live context and are in tests/test_gpu_plonk.py."""
import ctypes
import re
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, plonk
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["zkp_fr_prefix_product_dev", "zkp_fr_plonk_perm_z_dev", "zkp_fr_plonk_quotient_dev"]
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
    assert lib.zkp_version().startswith(b"zkp_accel 0.7.1")           # additive exports: the version string stays


def test_constants_agree_with_the_header():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "plonk.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (PLONK_[A-Z_]+) = (\d+);", hpp)}
    consts.pop("PLONK_SCAN_MAX_LOG")
    assert consts == {k: getattr(plonk, k) for k in ("PLONK_SCAN_THREADS", "PLONK_SCAN_ITEMS", "PLONK_SCAN_BLOCK", "PLONK_QUOT_THREADS",
                                                     "PLONK_QUOT_MAX_BLOCKS")}
    assert plonk.PLONK_SCAN_BLOCK == plonk.PLONK_SCAN_THREADS * plonk.PLONK_SCAN_ITEMS
    # the public header quotes the block size in the contract of zkp_fr_prefix_product_dev
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert f"a block of {plonk.PLONK_SCAN_BLOCK} consecutive elements" in text


def test_null_context_and_null_arrays_are_rejected():
    lib = _lib.load()
    fr = np.zeros((16, 4), dtype=np.uint64)
    fake = V(fr.ctypes.data)                                       # a non-NULL stand-in: a NULL context returns before any use
    four, seven = (V * 4)(fake, fake, fake, fake), (V * 7)(*[fake] * 7)
    closes = ctypes.c_int32(7)
    cl = ctypes.cast(ctypes.byref(closes), V)
    # NULL context
    assert lib.zkp_fr_prefix_product_dev(None, 0, fake, fake, 4, fake) == -1
    assert lib.zkp_fr_plonk_perm_z_dev(None, 0, four, four, 2, fake, fake, fake, fake, cl) == -1
    assert lib.zkp_fr_plonk_quotient_dev(None, 0, four, fake, fake, seven, four, fake, 2, fake, fake, fake, fake, fake) == -1
    # NULL arrays (checked before the context is touched, so a stand-in context is never dereferenced)
    assert lib.zkp_fr_prefix_product_dev(fake, 0, None, fake, 4, None) == -1
    assert lib.zkp_fr_prefix_product_dev(fake, 0, fake, None, 4, None) == -1
    perm = [four, four, 2, fake, fake, fake, fake, cl]
    for k in (0, 1, 3, 4, 5, 6, 7):
        args = list(perm)
        args[k] = None
        assert lib.zkp_fr_plonk_perm_z_dev(fake, 0, *args) == -1, k
    quot = [four, fake, fake, seven, four, fake, 2, fake, fake, fake, fake, fake]
    for k in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11):
        args = list(quot)
        args[k] = None
        assert lib.zkp_fr_plonk_quotient_dev(fake, 0, *args) == -1, k
    # a NULL entry inside an array of table pointers
    for k in range(4):
        holed = (V * 4)(*[None if i == k else fake for i in range(4)])
        assert lib.zkp_fr_plonk_perm_z_dev(fake, 0, holed, four, 2, fake, fake, fake, fake, cl) == -1
        assert lib.zkp_fr_plonk_perm_z_dev(fake, 0, four, holed, 2, fake, fake, fake, fake, cl) == -1
        assert lib.zkp_fr_plonk_quotient_dev(fake, 0, holed, fake, fake, seven, four, fake, 2, fake, fake, fake, fake, fake) == -1
        assert lib.zkp_fr_plonk_quotient_dev(fake, 0, four, fake, fake, seven, holed, fake, 2, fake, fake, fake, fake, fake) == -1
    for k in range(7):
        holed = (V * 7)(*[None if i == k else fake for i in range(7)])
        assert lib.zkp_fr_plonk_quotient_dev(fake, 0, four, fake, fake, holed, four, fake, 2, fake, fake, fake, fake, fake) == -1
    assert closes.value == 7
