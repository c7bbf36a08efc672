"""CPU: the Bulletproofs entry points are declared, exported, bound and present in the generated Rust declarations, their constants
agree between bulletproofs.hpp, bulletproofs.py and the numbers the public header quotes, zkp_bp_vectors has the C layout, and every
entry rejects a NULL context or NULL required pointers without dereferencing anything (no compute calls).  Every other argument rule
needs a live context and is in tests/test_gpu_bulletproofs.py."""
import ctypes
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, bulletproofs
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"zkp_fr_powers_dev": 6, "zkp_fr_bp_t_coeffs_dev": 6, "zkp_fr_bp_lr_eval_dev": 9, "zkp_fr_ipa_fold_ab_dev": 7}
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
    assert "pub struct zkp_bp_vectors {" in ffi
    # the version comment lists them among the entries detected by symbol
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert " / ".join(NAMES) in text[:text.index("const char* zkp_version(void);")]


def test_constants_agree():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "bulletproofs.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (BP_[A-Z_]+) = (\d+);", hpp)}
    assert consts == {"BP_THREADS": bulletproofs.BP_THREADS, "BP_MAX_GROUPS": bulletproofs.BP_MAX_GROUPS,
                      "BP_SUM_GROUP": bulletproofs.BP_SUM_GROUP}
    t = bulletproofs.BP_THREADS
    assert t & (t - 1) == 0 and 9 % bulletproofs.BP_SUM_GROUP == 0
    assert bulletproofs.BP_SUM_GROUP * t * 32 <= 64 * 1024       # one LDS buffer holds a group of sums
    assert int(re.search(r"constexpr int BP_MAX_LOG = (\d+);", hpp).group(1)) == 28
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    assert f"T = {t} * min(ceil(n / {t}), {bulletproofs.BP_MAX_GROUPS}) threads" in text
    assert "reduced three at a time" in text and bulletproofs.BP_SUM_GROUP == 3
    assert int(re.search(r"#define ZKP_MSM_SMALL_MAX_G1 (\d+)", text).group(1)) == bulletproofs.MSM_SMALL_MAX_G1


def test_bp_vectors_layout_matches_the_header():
    fields = [f[0] for f in _lib.BpVectors._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"zkp_accel.h\"\nint main(void){printf(\"%zu\", sizeof(zkp_bp_vectors));" + \
        "".join(f'printf(" %zu", offsetof(zkp_bp_vectors, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(prog)
        subprocess.run(["gcc", "-std=c99", f"-I{ROOT / 'include'}", str(Path(d) / "t.c"), "-o", str(Path(d) / "t")], check=True)
        nums = [int(x) for x in subprocess.run([str(Path(d) / "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(_lib.BpVectors)
    assert nums[1:] == [getattr(_lib.BpVectors, f).offset for f in fields]


def test_null_context_and_null_pointers_are_rejected():
    lib = _lib.load()
    fr = np.zeros((8, 4), dtype=np.uint64)
    fake = V(fr.ctypes.data)                                       # a non-NULL stand-in: a NULL context returns before any use
    vecs = _lib.BpVectors(None, None, None, None, None, None, None, 0, 0, 0, 1)
    pv = ctypes.byref(vecs)
    # NULL context
    assert lib.zkp_fr_powers_dev(None, 0, fake, fake, fake, 2) == -1
    assert lib.zkp_fr_powers_dev(None, 0, fake, fake, fake, 0) == -1
    assert lib.zkp_fr_bp_t_coeffs_dev(None, 0, pv, fake, fake, fake) == -1
    assert lib.zkp_fr_bp_lr_eval_dev(None, 0, pv, fake, fake, fake, fake, fake, fake) == -1
    assert lib.zkp_fr_ipa_fold_ab_dev(None, 0, fake, fake, 2, fake, fake) == -1
    # NULL required pointers (checked before the context is touched, so a stand-in context is never dereferenced)
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.zkp_fr_powers_dev(fake, 0, *args, 2) == -1
    for args in ((None, fake, fake, fake), (pv, None, fake, fake), (pv, fake, None, fake), (pv, fake, fake, None)):
        assert lib.zkp_fr_bp_t_coeffs_dev(fake, 0, *args) == -1
    full = [pv, fake, fake, fake, fake, fake, fake]
    for i in range(len(full)):
        args = list(full)
        args[i] = None
        assert lib.zkp_fr_bp_lr_eval_dev(fake, 0, *args) == -1, i
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.zkp_fr_ipa_fold_ab_dev(fake, 0, args[0], args[1], 2, args[2], fake) == -1
    assert (fr == 0).all()
