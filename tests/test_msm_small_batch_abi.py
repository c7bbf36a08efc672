"""CPU: the batched small variable-base MSM (zkp_msm_g*_var_batch_dev) is exported, declared with its caps, bound in Python,
and rejects a NULL context without touching a device."""
import ctypes
import re
from pathlib import Path

from ckb_zkp_amd import _lib
from ckb_zkp_amd.api import Context

ROOT = Path(__file__).resolve().parent.parent
SYMS = ("zkp_msm_g1_var_batch_dev", "zkp_msm_g2_var_batch_dev")


def test_symbols_exported_and_bound():
    lib = _lib.load()
    for s in SYMS:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    assert lib.zkp_version().startswith(b"zkp_accel 0.7")


def test_header_declares_caps():
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    caps = dict(re.findall(r"#define\s+(ZKP_MSM_SMALL_MAX_G[12])\s+(\d+)", text))
    assert int(caps["ZKP_MSM_SMALL_MAX_G1"]) == 1 << 16
    assert int(caps["ZKP_MSM_SMALL_MAX_G2"]) == 1 << 15
    for s in SYMS:
        assert re.search(r"int32_t\s+" + s + r"\s*\(", text), s


def test_python_methods_exist():
    assert callable(getattr(Context, "msm_var_batch_dev", None))
    assert callable(getattr(Context, "msm_var_batch", None))


def test_null_context_is_bad_arg():
    lib = _lib.load()
    one = (ctypes.c_size_t * 1)(4)
    ptrs = (ctypes.c_void_p * 1)(None)
    out = (ctypes.c_uint64 * 24)()
    for s in SYMS:
        fn = getattr(lib, s)
        assert fn(None, 0, 0, None, None, None, None, 0, None) == -1            # count == 0, NULL context
        assert fn(None, 0, 1, ptrs, None, ptrs, one, 0, out) == -1
        assert fn(None, 0, 1, None, None, None, None, 0, out) == -1              # count > 0 with NULL arrays
