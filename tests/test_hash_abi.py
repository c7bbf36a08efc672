"""CPU: the hash and Merkle entry points are declared, exported, bound and present in the generated Rust declarations, their
constants agree between fr_hash.hpp, the public header and the drivers, every entry rejects a NULL context or NULL required
pointers without dereferencing anything (no compute calls), and hashes.bytes_to_elements chunks as the reference does.  Every other
argument rule needs a live context and is in tests/test_gpu_hash.py / tests/test_gpu_merkle.py."""
import ctypes
import re
from pathlib import Path

import numpy as np

from ckb_zkp_amd import _lib, hashes, merkle
from ckb_zkp_amd.params import get_curve
from tests.test_abi import header_symbols

ROOT = Path(__file__).resolve().parent.parent
NAMES = {"zkp_hash_params_create": 4, "zkp_hash_params_free": 2, "zkp_hash_params_info": 2, "zkp_fr_hash_blocks_dev": 6,
         "zkp_fr_hash_chain_dev": 7, "zkp_fr_mimc_trace_dev": 7, "zkp_fr_merkle_tree_dev": 5, "zkp_fr_merkle_paths_dev": 8}
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
    for word in ("pub struct zkp_hash_desc", "pub struct zkp_hash_params", "ZKP_HASH_RESCUE", "ZKP_MERGE_CHAIN", "ZKP_MERKLE_BAD_LEAF",
                 "ZKP_HASH_MAX_LOG_LEAVES"):
        assert word in ffi, word
    # the version comment lists them among the entries detected by symbol, and the version stays
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    listed = " ".join(text[:text.index("const char* zkp_version(void);")].replace("*", " ").split())
    assert " / ".join(NAMES) in listed
    assert lib.zkp_version() == b"zkp_accel 0.7.1 (gfx950)"


def test_constants_agree():
    hpp = (ROOT / "ckb_zkp_amd" / "csrc" / "fr_hash.hpp").read_text()
    consts = {k: int(v) for k, v in re.findall(r"constexpr uint32_t (HASH_[A-Z_]+) = (\d+);", hpp)}
    assert consts == {"HASH_WIDTH": hashes.HASH_WIDTH, "HASH_THREADS": hashes.HASH_THREADS, "HASH_TAIL_NODES": hashes.HASH_TAIL_NODES,
                      "HASH_TAIL_DEPTHS": hashes.HASH_TAIL_DEPTHS, "HASH_RESCUE_WINDOW": hashes.HASH_RESCUE_WINDOW,
                      "HASH_MAX_ROUNDS_MIMC": hashes.HASH_MAX_ROUNDS_MIMC, "HASH_MAX_ROUNDS_POSEIDON": hashes.HASH_MAX_ROUNDS_POSEIDON,
                      "HASH_MAX_ROUNDS_RESCUE": hashes.HASH_MAX_ROUNDS_RESCUE, "HASH_MAX_LOG_BLOCKS": hashes.HASH_MAX_LOG_BLOCKS,
                      "HASH_MAX_LOG_LEAVES": hashes.HASH_MAX_LOG_LEAVES}
    assert "constexpr uint32_t HASH_TAIL_SPAN = 2 * HASH_TAIL_NODES - 1;" in hpp
    assert hashes.HASH_TAIL_NODES == 256 == 1 << (hashes.HASH_TAIL_DEPTHS - 1)
    text = (ROOT / "include" / "zkp_accel.h").read_text()
    defines = {k: int(v) for k, v in re.findall(r"#define (ZKP_(?:HASH|MERKLE)_[A-Z_]+) (\d+)", text)}
    assert defines == {"ZKP_HASH_WIDTH": hashes.HASH_WIDTH, "ZKP_HASH_MAX_ROUNDS_MIMC": hashes.HASH_MAX_ROUNDS_MIMC,
                       "ZKP_HASH_MAX_ROUNDS_POSEIDON": hashes.HASH_MAX_ROUNDS_POSEIDON,
                       "ZKP_HASH_MAX_ROUNDS_RESCUE": hashes.HASH_MAX_ROUNDS_RESCUE, "ZKP_HASH_MAX_LOG_BLOCKS": hashes.HASH_MAX_LOG_BLOCKS,
                       "ZKP_HASH_MAX_LOG_LEAVES": hashes.HASH_MAX_LOG_LEAVES, "ZKP_MERKLE_BAD_LEAF": merkle.BAD_LEAF}
    bodies = " ".join(re.findall(r"typedef enum \{([^}]*)\} zkp_(?:hash_kind|merge);", text))
    enums = dict(re.findall(r"(ZKP_[A-Z_]+) = (\d)", bodies))
    assert enums == {"ZKP_HASH_MIMC": str(hashes.KIND_MIMC), "ZKP_HASH_POSEIDON": str(hashes.KIND_POSEIDON),
                     "ZKP_HASH_RESCUE": str(hashes.KIND_RESCUE), "ZKP_MERGE_BLOCK": str(merkle.MERGE_BLOCK),
                     "ZKP_MERGE_CHAIN": str(merkle.MERGE_CHAIN)}
    # the largest constant table the design stages nowhere: MiMC's cap, 32 bytes a round
    assert hashes.HASH_MAX_ROUNDS_MIMC >= 322 and hashes.HASH_MAX_ROUNDS_POSEIDON >= 91 and hashes.HASH_MAX_ROUNDS_RESCUE >= 22


def test_desc_layout_matches_the_header():
    import subprocess
    import tempfile
    fields = [f[0] for f in _lib.HashDesc._fields_]
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"zkp_accel.h\"\nint main(void){printf(\"%zu\", sizeof(zkp_hash_desc));" + \
        "".join(f'printf(" %zu", offsetof(zkp_hash_desc, {f}));' for f in fields) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "t.c").write_text(prog)
        subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", f"-I{ROOT / 'include'}", str(Path(d) / "t.c"), "-o", str(Path(d) / "t")],
                       check=True)
        nums = [int(x) for x in subprocess.run([str(Path(d) / "t")], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == ctypes.sizeof(_lib.HashDesc)
    assert nums[1:] == [getattr(_lib.HashDesc, f).offset for f in fields]


def test_null_context_and_null_pointers_are_rejected():
    lib = _lib.load()
    fr = np.zeros((8, 4), dtype=np.uint64)
    idx = np.zeros(4, dtype=np.uint32)
    fake, p = V(fr.ctypes.data), V(idx.ctypes.data)       # non-NULL stand-ins: never dereferenced before the rejection
    desc = _lib.HashDesc(ctypes.sizeof(_lib.HashDesc), 0, 1, 0, fake, None, None)
    out = V()
    # NULL context
    assert lib.zkp_hash_params_create(None, 0, ctypes.byref(desc), ctypes.byref(out)) == -1 and not out.value
    assert lib.zkp_hash_params_free(None, fake) == -1
    assert lib.zkp_fr_hash_blocks_dev(None, fake, fake, fake, 1, fake) == -1
    assert lib.zkp_fr_hash_chain_dev(None, fake, fake, 1, 1, fake, fake) == -1
    assert lib.zkp_fr_mimc_trace_dev(None, fake, fake, fake, 1, fake, 12) == -1
    assert lib.zkp_fr_merkle_tree_dev(None, fake, 0, fake, 2) == -1
    assert lib.zkp_fr_merkle_paths_dev(None, fake, 2, p, 1, fake, 1, p) == -1
    # NULL required pointers (checked before the context is touched, so a stand-in context is never dereferenced)
    assert lib.zkp_hash_params_create(fake, 0, None, ctypes.byref(out)) == -1
    assert lib.zkp_hash_params_create(fake, 0, ctypes.byref(desc), None) == -1
    assert lib.zkp_hash_params_free(fake, None) == -1
    assert lib.zkp_hash_params_info(None, fr.ctypes.data_as(_lib.u64p)) == -1
    assert lib.zkp_hash_params_info(fake, None) == -1
    for a in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert lib.zkp_fr_hash_blocks_dev(fake, a[0], a[1], a[2], 1, a[3]) == -1
        assert lib.zkp_fr_mimc_trace_dev(fake, a[0], a[1], a[2], 1, a[3], 12) == -1
    for a in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.zkp_fr_hash_chain_dev(fake, a[0], a[1], 1, 1, a[2], None) == -1
    assert lib.zkp_fr_merkle_tree_dev(fake, None, 0, fake, 2) == -1
    assert lib.zkp_fr_merkle_tree_dev(fake, fake, 0, None, 2) == -1
    for a in ((None, p, fake, p), (fake, None, fake, p), (fake, p, None, p), (fake, p, fake, None)):
        assert lib.zkp_fr_merkle_paths_dev(fake, a[0], 2, a[1], 1, a[2], 1, a[3]) == -1
    assert (fr == 0).all() and (idx == 0).all()


def test_bytes_to_elements_chunks_as_the_reference_does():
    for curve in ("bn254", "bls12_381"):
        r = get_curve(curve).r
        assert hashes.bytes_to_elements(b"", curve) == []
        full = (5).to_bytes(32, "little") + (r - 1).to_bytes(32, "little")
        assert hashes.bytes_to_elements(full, curve) == [5, r - 1]                         # an empty tail adds nothing
        assert hashes.bytes_to_elements(full + b"\x01\x02", curve) == [5, r - 1, 0x0201]   # a partial tail is zero-extended
        assert hashes.bytes_to_elements(b"\xff" * 31, curve) == [(1 << 248) - 1]
        for big in (r, r + 1, (1 << 256) - 1):                                             # no canonical element: 0
            assert hashes.bytes_to_elements((7).to_bytes(32, "little") + big.to_bytes(32, "little"), curve) == [7, 0]
