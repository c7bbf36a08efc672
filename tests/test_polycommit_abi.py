"""CPU: the Pedersen / polynomial-commitment entry points are declared, exported, bound and present in the generated Rust
declarations with the same arity, their constants agree between pedersen.hpp, polycommit.py and the public header, and every entry
rejects a NULL context or NULL required pointers without dereferencing anything (no compute calls).  Every other argument rule
needs a live context and is in tests/test_gpu_pedersen.py / tests/test_gpu_vecmat.py."""
import ctypes
import re
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, polycommit
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"zkp_pedersen_key_create": 7, "zkp_pedersen_key_free": 2, "zkp_pedersen_key_info": 2, "zkp_pedersen_commit_rows_dev": 8,
         "zkp_fr_vecmat_dev": 7}
V = ctypes.c_void_p


def test_symbols_exported_declared_and_bound():
    lib = _lib.load()
    declared = header_symbols()
    ffi = (ROOT / "rust" / "zkp-accel" / "src" / "ffi.rs").read_text()
    for name, arity in NAMES.items():
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        m = re.search(rf"pub fn {name}\(([^)]*)\)", ffi)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
        assert len(_lib.SIGNATURES[name][1]) == arity, name
    assert "ZKP_PEDERSEN_MAX_GENS" in ffi and "ZKP_FR_VECMAT_ROW_CHUNK" in ffi and "pub struct zkp_pedersen_key" in ffi
    # the version comment lists them among the entries detected by symbol
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert " / ".join(NAMES) in text[:text.index("const char* zkp_version(void);")]


def test_constants_agree():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "pedersen.hpp").read_text()
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert define("ZKP_PEDERSEN_MAX_GENS") == polycommit.PEDERSEN_MAX_GENS == define("ZKP_MSM_SMALL_MAX_G1")
    assert define("ZKP_FR_VECMAT_ROW_CHUNK") == polycommit.VECMAT_ROW_CHUNK
    assert f"constexpr uint32_t PED_MAX_GENS = {polycommit.PEDERSEN_MAX_GENS};" in hpp
    assert f"constexpr uint32_t VECMAT_ROW_CHUNK = {polycommit.VECMAT_ROW_CHUNK};" in hpp
    assert f"constexpr int PED_LANES = {polycommit.PEDERSEN_ROW_LANES};" in hpp
    assert "constexpr uint64_t PED_MAX_CELLS = (uint64_t)1 << 28;" in hpp and polycommit.MAX_CELLS == 1 << 28
    assert "rows * cols <= 2^28" in text
    assert polycommit.split_sizes(20) == (1 << 10, 1 << 10) and polycommit.split_sizes(5) == (4, 8) and polycommit.split_sizes(0) == (1, 1)


def test_null_context_and_null_pointers_are_rejected():
    lib = _lib.load()
    buf = np.zeros((8, 12), dtype=np.uint64)
    fake = V(buf.ctypes.data)                                        # a non-NULL stand-in: a NULL context returns before any use
    out = V()
    assert lib.zkp_pedersen_key_create(None, 0, fake, None, 1, fake, ctypes.byref(out)) == -1
    assert lib.zkp_pedersen_key_free(None, fake) == -1
    assert lib.zkp_pedersen_commit_rows_dev(None, fake, fake, 1, 1, None, fake, fake) == -1
    assert lib.zkp_fr_vecmat_dev(None, 0, fake, fake, 1, 1, fake) == -1
    # NULL required pointers (checked before the context is touched, so a stand-in context is never dereferenced)
    for args in ((None, fake, ctypes.byref(out)), (fake, None, ctypes.byref(out)), (fake, fake, None)):
        assert lib.zkp_pedersen_key_create(fake, 0, args[0], None, 1, args[1], args[2]) == -1
    assert lib.zkp_pedersen_key_free(fake, None) == -1
    info = (ctypes.c_uint64 * 8)()
    assert lib.zkp_pedersen_key_info(None, info) == -1 and lib.zkp_pedersen_key_info(fake, None) == -1
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert lib.zkp_pedersen_commit_rows_dev(fake, args[0], args[1], 1, 1, None, args[2], args[3]) == -1
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.zkp_fr_vecmat_dev(fake, 0, args[0], args[1], 1, 1, args[2]) == -1
    assert out.value is None and (buf == 0).all() and not any(info)
