"""CPU: zkp_fr_poly_eval_many_dev / zkp_fr_lincomb_dev are declared, exported and bound, their constants agree between fr_open.hpp
and plonk.py, and both reject a NULL context, NULL arrays and a NULL vector with a length without dereferencing anything (no
compute calls).  The rules that need a live context are in tests/test_gpu_plonk_open.py."""
import ctypes
import re
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, api, plonk
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["zkp_fr_poly_eval_many_dev", "zkp_fr_lincomb_dev"]
V = ctypes.c_void_p


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    declared = header_symbols()
    ffi = (ROOT / "rust" / "zkp-accel" / "src" / "ffi.rs").read_text()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert f"pub fn {name}(" in ffi, name
        assert hasattr(api.Context, name[len("zkp_"):]), name
    assert lib.zkp_version().startswith(b"zkp_accel 0.7.1")           # additive exports: the version string stays


def test_constants_agree_with_the_header():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "fr_open.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (FR_OPEN_[A-Z_]+) = (\d+);", hpp)}
    assert consts.pop("FR_OPEN_MAX_LOG") == 30 and consts.pop("FR_OPEN_LINCOMB_THREADS") == 256
    names = ("FR_OPEN_MAX_POLYS", "FR_OPEN_EVAL_THREADS", "FR_OPEN_EVAL_MAX_BLOCKS", "FR_OPEN_EVAL_GROUP")
    assert consts == {k: getattr(plonk, k) for k in names}
    assert plonk.FR_OPEN_MAX_POLYS == 32 and plonk.FR_OPEN_MAX_POLYS % plonk.FR_OPEN_EVAL_GROUP == 0
    # the evaluation's launch rule is the quotient kernel's
    assert (plonk.FR_OPEN_EVAL_THREADS, plonk.FR_OPEN_EVAL_MAX_BLOCKS) == (plonk.PLONK_QUOT_THREADS, plonk.PLONK_QUOT_MAX_BLOCKS)
    # the 20 polynomials of rounds 4 and 5 fit one call
    assert len(plonk.BASE_POLYS) == 20 <= plonk.FR_OPEN_MAX_POLYS
    # the public header quotes the limits in the contract
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert f"1 <= count <= {plonk.FR_OPEN_MAX_POLYS}" in text
    assert f"T = {plonk.FR_OPEN_EVAL_THREADS} * min(ceil(max ns / {plonk.FR_OPEN_EVAL_THREADS}), {plonk.FR_OPEN_EVAL_MAX_BLOCKS})" in text
    assert f"register groups of {plonk.FR_OPEN_EVAL_GROUP}" in text


def test_null_context_and_null_arrays_are_rejected():
    lib = _lib.load()
    fr = np.zeros((16, 4), dtype=np.uint64)
    fake = V(fr.ctypes.data)                                       # a non-NULL stand-in: a NULL context returns before any use
    out = np.full((4, 4), 7, dtype=np.uint64)
    outp = V(out.ctypes.data)
    three = (V * 3)(fake, fake, fake)
    ns = (ctypes.c_size_t * 3)(4, 4, 4)
    ev = [3, three, ns, fake, outp]
    lc = [3, three, ns, fake, outp, 4]
    # NULL context
    assert lib.zkp_fr_poly_eval_many_dev(None, 0, *ev) == -1
    assert lib.zkp_fr_lincomb_dev(None, 0, *lc) == -1
    # NULL arrays (checked before the context is touched, so a stand-in context is never dereferenced)
    for k in (1, 2, 3, 4):
        args = list(ev)
        args[k] = None
        assert lib.zkp_fr_poly_eval_many_dev(fake, 0, *args) == -1, k
        args = list(lc)
        args[k] = None
        assert lib.zkp_fr_lincomb_dev(fake, 0, *args) == -1, k
    # a NULL entry inside the pointer array with ns[k] > 0
    for k in range(3):
        holed = (V * 3)(*[None if i == k else fake for i in range(3)])
        assert lib.zkp_fr_poly_eval_many_dev(fake, 0, 3, holed, ns, fake, outp) == -1, k
        assert lib.zkp_fr_lincomb_dev(fake, 0, 3, holed, ns, fake, outp, 4) == -1, k
    assert (out == 7).all() and not fr.any()
