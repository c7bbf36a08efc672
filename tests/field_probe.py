"""Builds tests/hip/*.hip into tests/hip/build/libzkp_field_probe.so and runs it: a test-only probe that puts every primitive of
the device arithmetic (field_dev.hpp, unsat_dev.hpp, bucket_dev.hpp, coop_dev.hpp, ec_dev.hpp) behind its own one-lane-per-case kernel.

The product headers are included unchanged and compiled with the flags of ckb_zkp_amd/build.py (FLAGS + UNROLL, default macros).
ZKP_PROBE_CSRC=<dir> takes the headers from another directory and builds into build/<ZKP_PROBE_TAG or "alt">/ (sensitivity runs
against a mutated copy of the headers); the shipped probe is the build without it.

    python -m tests.field_probe [--force]
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
HIP = ROOT / "tests" / "hip"
CSRC = Path(os.environ["ZKP_PROBE_CSRC"]).resolve() if os.environ.get("ZKP_PROBE_CSRC") else ROOT / "ckb_zkp_amd" / "csrc"
_ALT = "ZKP_PROBE_CSRC" in os.environ and bool(os.environ["ZKP_PROBE_CSRC"])
OUTDIR = HIP / "build" / (os.environ.get("ZKP_PROBE_TAG", "alt") if _ALT else "")
OBJDIR = OUTDIR / "obj"
LIB = OUTDIR / "libzkp_field_probe.so"
MAX_JOBS = 16

FIELDS = {"Bn254Fq": 0, "Bn254Fr": 1, "Bls381Fq": 2, "Bls381Fr": 3}

# (source, object, extra flags)
UNITS = [("field_probe.hip", "field_probe.o", []),
         ("probe_fp.hip", "probe_fp_inline.o", ["-DZKP_INLINE_MUL", "-DPROBE_FP_ENTRY=probe_fp_inline"]),
         ("probe_fp.hip", "probe_fp_outline.o", ["-DPROBE_FP_ENTRY=probe_fp_outline"]),
         ("probe_fu.hip", "probe_fu_9.o", ["-DPROBE_FU_PART=0", "-DPROBE_FU_ENTRY=probe_fu_9"]),
         ("probe_fu.hip", "probe_fu_14.o", ["-DPROBE_FU_PART=1", "-DPROBE_FU_ENTRY=probe_fu_14"])]
for _c in (0, 1):
    UNITS.append(("probe_g1.hip", f"probe_g1_c{_c}.o", [f"-DPROBE_CURVE={_c}", f"-DPROBE_G1_ENTRY=probe_g1_c{_c}"]))
    for _p in (0, 1):
        UNITS.append(("probe_g2.hip", f"probe_g2_c{_c}_p{_p}.o",
                      [f"-DPROBE_CURVE={_c}", f"-DPROBE_G2_PART={_p}", f"-DPROBE_G2_ENTRY=probe_g2_c{_c}_p{_p}"]))
# ec_dev.hpp: one object per curve x group x part, the multiplier inlined where the product's msm_group unit inlines it (build.py)
for _c in (0, 1):
    for _g in (1, 2):
        for _p in range(4):
            UNITS.append(("probe_ec.hip", f"probe_ec_c{_c}_g{_g}_p{_p}.o",
                          [f"-DPROBE_CURVE={_c}", f"-DPROBE_GROUP={_g}", f"-DPROBE_EC_PART={_p}", f"-DPROBE_EC_ENTRY=probe_ec_c{_c}_g{_g}_p{_p}"]
                          + (["-DZKP_INLINE_MUL"] if (_c, _g) != (1, 2) else [])))


def _deps():
    return sorted(CSRC.glob("*.hpp")) + sorted(CSRC.glob("*.inc")) + sorted(HIP.glob("*.hpp")) + [Path(__file__)]


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile what is older than its sources or the headers; returns the library.  At most 16 compile jobs."""
    from ckb_zkp_amd import build as pb
    deps = _deps()
    if not force and pb._newer(LIB, [HIP / u[0] for u in UNITS] + deps):    # up to date: the objects need not be there
        return LIB
    OBJDIR.mkdir(parents=True, exist_ok=True)
    hipcc = pb._hipcc()
    flags = [*pb.FLAGS, *pb.UNROLL, f"-I{CSRC}", f"-I{HIP}"]

    def compile_one(unit):
        src, oname, extra = unit
        s, o = HIP / src, OBJDIR / oname
        if not force and pb._newer(o, [s, *deps]):
            return o, 0.0
        t0 = time.time()
        r = subprocess.run([hipcc, *flags, *extra, "-c", str(s), "-o", str(o)], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src} {extra}:\n{r.stdout}\n{r.stderr}")
        if "warning" in r.stderr:
            print(f"[probe] {oname}: compiler warnings\n{r.stderr}", file=sys.stderr)
        return o, time.time() - t0

    with ThreadPoolExecutor(max_workers=min(len(UNITS), MAX_JOBS, os.cpu_count() or 4)) as ex:
        results = list(ex.map(compile_one, UNITS))
    if verbose:
        for (o, dt), u in zip(results, UNITS):
            print(f"[probe] {u[1]}: {'cached' if dt == 0 else '%.1fs' % dt}", file=sys.stderr)
    objs = [o for o, _ in results]
    if force or not pb._newer(LIB, objs):
        r = subprocess.run([hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", str(LIB), *map(str, objs)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return LIB


_lib = None


def load():
    global _lib
    if _lib is None:
        lib = ctypes.CDLL(str(build()))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        lib.zkp_probe_run.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, u32p, ctypes.c_int, u32p, ctypes.c_int]
        lib.zkp_probe_run.restype = ctypes.c_int
        _lib = lib
    return _lib


def run(device: int, op: str, field: str, inp: np.ndarray, out: np.ndarray) -> np.ndarray:
    """One lane (or quad) per row of `inp`; `out` (same number of rows) is sent to the device and comes back overwritten."""
    inp = np.ascontiguousarray(inp, dtype=np.uint32)
    out = np.ascontiguousarray(out, dtype=np.uint32).copy()
    assert inp.ndim == 2 and out.ndim == 2 and inp.shape[0] == out.shape[0] and inp.shape[1] >= 1
    u32p = ctypes.POINTER(ctypes.c_uint32)
    st = load().zkp_probe_run(device, op.encode(), FIELDS[field], inp.shape[0], inp.ctypes.data_as(u32p), inp.shape[1],
                              out.ctypes.data_as(u32p), out.shape[1])
    if st != 0:
        raise RuntimeError(f"zkp_probe_run({op}, {field}) -> {st}")
    return out


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    print(build(force="--force" in sys.argv, verbose=True))
