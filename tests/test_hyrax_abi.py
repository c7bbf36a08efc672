"""CPU: the Hyrax entry points are declared, exported, bound and present in the generated Rust declarations, their constants agree
between hyrax.hpp and hyrax.py, and both entries reject a NULL context or NULL arrays without dereferencing anything (no compute
calls).  Every other argument rule needs a live context and is in tests/test_gpu_hyrax.py."""
import ctypes
import re
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, hyrax
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = ["zkp_fr_gkr_eval_layer_batch_dev", "zkp_fr_gkr_dp_round_dev"]
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
    assert len(_lib.SIGNATURES["zkp_fr_gkr_eval_layer_batch_dev"][1]) == 6
    assert len(_lib.SIGNATURES["zkp_fr_gkr_dp_round_dev"][1]) == 11


def test_constants_agree_with_the_header():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "hyrax.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (HYRAX_[A-Z]+) = (\d+);", hpp)}
    assert consts == {"HYRAX_THREADS": hyrax.HYRAX_THREADS, "HYRAX_CHUNK": hyrax.HYRAX_CHUNK}
    assert hyrax.HYRAX_THREADS & (hyrax.HYRAX_THREADS - 1) == 0 and hyrax.HYRAX_CHUNK >= 2
    # the public header quotes both numbers in the contract of zkp_fr_gkr_dp_round_dev
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert f"chunks of {hyrax.HYRAX_CHUNK} entries, one workgroup per {hyrax.HYRAX_THREADS} columns and chunk" in text
    assert f"ceil(columns / {hyrax.HYRAX_THREADS}) * ceil(n_gates / {hyrax.HYRAX_CHUNK})" in text


def test_null_context_and_null_arrays_are_rejected():
    lib = _lib.load()
    fr = np.zeros((8, 4), dtype=np.uint64)
    fake = V(fr.ctypes.data)                                       # a non-NULL stand-in: a NULL context returns before any use
    # NULL context
    assert lib.zkp_fr_gkr_eval_layer_batch_dev(None, 0, fake, fake, fake, 2) == -1
    assert lib.zkp_fr_gkr_dp_round_dev(None, 0, fake, fake, fake, fake, 2, 2, fake, fake, None) == -1
    # NULL arrays / handles (checked before the context is touched, so a stand-in context is never dereferenced)
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.zkp_fr_gkr_eval_layer_batch_dev(fake, 0, *args, 2) == -1
    for args in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert lib.zkp_fr_gkr_dp_round_dev(fake, 0, *args, 2, 2, fake, fake, None) == -1
    assert lib.zkp_fr_gkr_dp_round_dev(fake, 0, fake, fake, fake, fake, 2, 2, None, None, None) == -1
    assert (fr == 0).all()
