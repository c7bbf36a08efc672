"""CPU: the aliasing rules of the entry points that write through caller pointers (ckb_zkp_amd/csrc/mem_spans.hpp, used through
fr_dev.hpp by gkr.hip, hyrax.hip, spark.hip, bulletproofs.hip, plonk.hip and fr_open.hip).  tests/c/mem_spans.cpp includes that
header alone and compares outputs_disjoint with its definition (two spans conflict iff both are non-empty, at least one is an
output and they intersect) over every set of up to 4 spans with end points in 0..6 and either flag, over random sets of up to 12
spans and over the named edge cases (empty spans, equal starts in both insertion orders, nesting both ways, touching spans),
and same_or_disjoint with its definition over every pair of short vectors."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
SRC = ROOT / "tests" / "c" / "mem_spans.cpp"
OUT = ROOT / "tests" / "c" / "build" / "mem_spans"


def test_the_predicates_agree_with_their_definitions():
    OUT.parent.mkdir(parents=True, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{CSRC}", str(SRC), "-o", str(OUT)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(OUT)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > 56 ** 4 + 6000
