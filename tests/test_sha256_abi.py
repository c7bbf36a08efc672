"""CPU: the SHA-256 entry points are declared, exported, bound and present in the generated Rust declarations; the layout of the
canonical trace and the caps agree between sha256.hpp, the public header, zkp_sha256_info and the drivers; every entry rejects a
NULL context or a NULL required pointer without dereferencing anything (no compute calls).  Every other argument rule needs a
live context and is in tests/test_gpu_sha256.py / tests/test_gpu_bits_expand.py."""
import ctypes
import re
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, bits
from ckb_zkp_amd import sha256 as S
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"zkp_sha256_info": 1, "zkp_sha256_dev": 5, "zkp_sha256_trace_dev": 5, "zkp_sha256_merkle_tree_dev": 3, "zkp_fr_bits_expand_dev": 11}
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
    assert "ZKP_SHA256_BLOCK_WORDS" in ffi and "ZKP_SHA256_MAX_LOG_CODE_WORDS" in ffi
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    listed = " ".join(text[:text.index("const char* zkp_version(void);")].replace("*", " ").split())
    assert " / ".join(NAMES) in listed
    assert lib.zkp_version() == b"zkp_accel 0.7.1 (gfx950)"


def test_layout_and_caps_agree():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "sha256.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (SHA256_[A-Z_]+) = (\d+);", hpp)}
    want = {"SHA256_BLOCK_WORDS": S.BLOCK_WORDS, "SHA256_OFF_INPUT": S.OFF_INPUT, "SHA256_OFF_SCHED": S.OFF_SCHED,
            "SHA256_SCHED_WORDS": S.SCHED_WORDS, "SHA256_OFF_ROUND": S.OFF_ROUND, "SHA256_ROUND_WORDS": S.ROUND_WORDS,
            "SHA256_OFF_FINAL": S.OFF_FINAL, "SHA256_THREADS": S.THREADS, "SHA256_EXPAND_THREADS": S.EXPAND_THREADS,
            "SHA256_MAX_LOG_LEN": S.MAX_LOG_LEN, "SHA256_MAX_LOG_BYTES": S.MAX_LOG_BYTES,
            "SHA256_MAX_LOG_TRACE_WORDS": S.MAX_LOG_TRACE_WORDS, "SHA256_MAX_LOG_LEAVES": S.MAX_LOG_LEAVES,
            "SHA256_MAX_LOG_CODE_WORDS": S.MAX_LOG_CODE_WORDS}
    assert consts == want
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    defines = {k: int(v) for k, v in re.findall(r"#define (ZKP_SHA256_[A-Z_]+) (\d+)", text)}
    assert defines == {"ZKP_" + k: v for k, v in want.items() if k == "SHA256_BLOCK_WORDS" or "_MAX_" in k}
    # what the library itself reports
    info = S.info()
    assert info == {"block_words": S.BLOCK_WORDS, "off_input": S.OFF_INPUT, "off_sched": S.OFF_SCHED, "sched_words": S.SCHED_WORDS,
                    "off_round": S.OFF_ROUND, "round_words": S.ROUND_WORDS, "off_final": S.OFF_FINAL, "max_log_len": S.MAX_LOG_LEN,
                    "max_log_bytes": S.MAX_LOG_BYTES, "max_log_trace_words": S.MAX_LOG_TRACE_WORDS, "max_log_leaves": S.MAX_LOG_LEAVES,
                    "max_log_code_words": S.MAX_LOG_CODE_WORDS, "threads": S.THREADS, "expand_threads": S.EXPAND_THREADS}
    # the four parts of a block record fill it, and a code has room for every word the caps allow
    assert S.OFF_SCHED == 16 and S.OFF_ROUND == S.OFF_SCHED + 48 * S.SCHED_WORDS and S.OFF_FINAL == S.OFF_ROUND + 64 * S.ROUND_WORDS
    assert S.BLOCK_WORDS == S.OFF_FINAL + 16
    assert bits.CODE_WORD_BITS == S.MAX_LOG_CODE_WORDS == 26 and bits.code((1 << 26) - 1, 31, 1) == 0xFFFFFFFF
    assert [S.blocks(n) for n in (0, 55, 56, 64, 119, 120)] == [1, 1, 2, 2, 2, 3] and S.trace_words(64) == 2049


def test_null_context_and_null_pointers_are_rejected():
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    fake = V(buf.ctypes.data)                              # a non-NULL stand-in: never dereferenced before the rejection
    assert lib.zkp_sha256_info(None) == -1
    # NULL context
    assert lib.zkp_sha256_dev(None, fake, 1, 64, fake) == -1
    assert lib.zkp_sha256_trace_dev(None, fake, 1, 64, fake) == -1
    assert lib.zkp_sha256_merkle_tree_dev(None, fake, 2) == -1
    assert lib.zkp_fr_bits_expand_dev(None, 0, fake, 2049, 1, 1, fake, 1, 0, fake, 1) == -1
    # NULL required pointers, checked before the context is touched
    for a in ((None, fake), (fake, None)):
        assert lib.zkp_sha256_dev(fake, a[0], 1, 64, a[1]) == -1
        assert lib.zkp_sha256_trace_dev(fake, a[0], 1, 64, a[1]) == -1
    assert lib.zkp_sha256_merkle_tree_dev(fake, None, 2) == -1
    for a in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.zkp_fr_bits_expand_dev(fake, 0, a[0], 2049, 1, 1, a[1], 1, 0, a[2], 1) == -1
    assert (buf == 0).all()
