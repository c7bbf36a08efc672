"""CPU: the aSVC entry points are declared, exported, bound and present in the generated Rust declarations, their constants agree
between asvc.hpp, asvc.py and the public header, and both entries reject a NULL context or NULL required pointers without
dereferencing anything (no compute calls).  Every other argument rule needs a live context and is in tests/test_gpu_asvc.py."""
import ctypes
import re
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, asvc
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"zkp_fr_asvc_subset_weights_dev": 7, "zkp_fr_asvc_quotient_dev": 7}
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
    assert "ZKP_ASVC_MAX_POSITIONS" in ffi
    # the version comment lists them among the entries detected by symbol
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert " / ".join(NAMES) in text[:text.index("const char* zkp_version(void);")]


def test_constants_agree():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "asvc.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (ASVC_[A-Z_]+) = (\d+);", hpp)}
    assert consts == {"ASVC_MAX_POSITIONS": asvc.ASVC_MAX_POSITIONS, "ASVC_THREADS": asvc.ASVC_THREADS, "ASVC_GROUP": asvc.ASVC_GROUP,
                      "ASVC_SPAN": asvc.ASVC_SPAN, "ASVC_CHUNK": asvc.ASVC_CHUNK, "ASVC_MAX_LOG": asvc.ASVC_MAX_LOG}
    assert "constexpr uint32_t ASVC_TILE = ASVC_CHUNK * ASVC_THREADS;" in hpp and asvc.ASVC_TILE == asvc.ASVC_CHUNK * asvc.ASVC_THREADS
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert int(re.search(r"#define ZKP_ASVC_MAX_POSITIONS (\d+)", text).group(1)) == asvc.ASVC_MAX_POSITIONS
    assert asvc.ASVC_MAX_POSITIONS * 64 <= 64 * 1024                 # w_i and c_i of every position: 64 B each, 64 KiB in all
    assert asvc.ASVC_THREADS * 32 <= 64 * 1024                       # the LDS buffer of a workgroup scan
    assert "four positions\n * share each coefficient load" in text and asvc.ASVC_GROUP == 4
    assert "accumulates eight consecutive q[t] per thread" in text and asvc.ASVC_SPAN == 8
    assert [asvc.segment_length(k) for k in (1, 2, 3, 4, 7, 8, 1023, 1024)] == [1, 2, 2, 4, 4, 8, 512, 1024]


def test_null_context_and_null_pointers_are_rejected():
    lib = _lib.load()
    fr = np.zeros((8, 4), dtype=np.uint64)
    pos = np.array([0, 1], dtype=np.uint32)
    fake, p = V(fr.ctypes.data), V(pos.ctypes.data)                  # non-NULL stand-ins: a NULL context returns before any use
    # NULL context
    assert lib.zkp_fr_asvc_subset_weights_dev(None, 0, 3, p, 2, fake, fake) == -1
    assert lib.zkp_fr_asvc_quotient_dev(None, 0, fake, 3, p, 2, fake) == -1
    # NULL required pointers (checked before the context is touched, so a stand-in context is never dereferenced)
    assert lib.zkp_fr_asvc_subset_weights_dev(fake, 0, 3, None, 2, fake, fake) == -1
    assert lib.zkp_fr_asvc_subset_weights_dev(fake, 0, 3, p, 2, None, None) == -1
    for args in ((None, p, fake), (fake, None, fake), (fake, p, None)):
        assert lib.zkp_fr_asvc_quotient_dev(fake, 0, args[0], 3, args[1], 2, args[2]) == -1
    assert (fr == 0).all() and list(pos) == [0, 1]
