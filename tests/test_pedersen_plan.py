"""CPU: the plan of the Pedersen bucket pass (ckb_zkp_amd/csrc/pedersen.hpp, used by pedersen.hip).  tests/c/pedersen_plan.cpp
includes that header alone and prints the plan of one (curve, cols) per run; here every plan is compared with a Python restatement
and checked against what the kernel relies on: the slices of a row cover every (generator, window) pair exactly once, a slice holds
at most 4096 pairs (12 bits of a sorted entry), the LDS of a workgroup fits a CDNA4 compute unit, and W c > 256 so the top window
absorbs the last carry."""
import os
import subprocess
from pathlib import Path

import pytest

from ckb_zkp_amd import polycommit

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
SRC = ROOT / "tests" / "c" / "pedersen_plan.cpp"
OUT = ROOT / "tests" / "c" / "build" / "pedersen_plan"
SMALL_LDS_MAX = 160 * 1024
BK_BYTES = {0: 4 * 4 * 9, 1: 4 * 4 * 14}       # BkPoint: 4 elements of 9 x 29-bit / 14 x 28-bit limbs


def model(curve, cols):
    c = 8
    W = (256 + c) // c
    nb = 1 << (c - 1)
    G = 4096 // W
    S = -(-cols // G)
    g = -(-cols // S)
    E = G * W
    lds = (nb + 128 + 64) * BK_BYTES[curve] + 4 * 128 + 4 * (nb + 4) + 4 * E + 2 * E
    return dict(c=c, W=W, nb=nb, G=G, S=S, g=g, lds_bytes=lds, bk_bytes=BK_BYTES[curve], lanes=64, slots=128, max_entries=4096,
                max_gens=65536, lds_max=SMALL_LDS_MAX, launches=3, row_chunk=32, vecmat_threads=64)


@pytest.fixture(scope="module")
def prog():
    OUT.parent.mkdir(parents=True, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{CSRC}", str(SRC), "-o", str(OUT)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(OUT)


def plan_of(prog, curve, cols):
    r = subprocess.run([prog, str(curve), str(cols)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (curve, cols, r.stdout, r.stderr)
    return {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}


@pytest.mark.parametrize("curve", [0, 1])
def test_plan_matches_the_model_and_keeps_its_bounds(prog, curve):
    G = plan_of(prog, curve, 1)["G"]
    for n_gens in (1, 2, G - 1, G, G + 1, 2 * G, 65536):
        p = plan_of(prog, curve, n_gens)
        assert p == model(curve, n_gens), (curve, n_gens)
        assert p["W"] * p["c"] > 256 and (p["W"] - 1) * p["c"] <= 256 and p["W"] <= p["lanes"]
        assert p["nb"] == 1 << (p["c"] - 1) and p["nb"] % p["lanes"] == 0
        assert p["g"] <= p["G"] and p["g"] * p["W"] <= p["max_entries"] and p["G"] * p["W"] <= p["max_entries"] < 1 << 15
        assert p["lds_bytes"] <= SMALL_LDS_MAX == p["lds_max"]
        # slice j covers generators [j g, min(cols, (j + 1) g)) in all W windows: every pair exactly once, no empty slice
        seen = [0] * n_gens
        for j in range(p["S"]):
            lo, hi = j * p["g"], min(n_gens, (j + 1) * p["g"])
            assert lo < hi, (curve, n_gens, j)
            for k in range(lo, hi):
                seen[k] += 1
        assert seen == [1] * n_gens, (curve, n_gens)
        assert p["max_gens"] == 65536 and n_gens <= p["max_gens"]


@pytest.mark.parametrize("curve", [0, 1])
def test_rows_of_more_slices_than_the_row_pass_has_lanes(prog, curve):
    """cols at which a lane of the row pass (ped_row_kernel: slices t, t + lanes, ...) takes a second slice, and the key cap, where
    a lane takes nine: the last row of one slice per lane, one generator more (the plan balances: S = lanes + 1 slices of g < G),
    one slice more, PED_MAX_GENS.  tests/test_gpu_pedersen.py runs these shapes on the device."""
    one = plan_of(prog, curve, 1)
    G, lanes, cap = one["G"], one["lanes"], one["max_gens"]
    assert lanes == polycommit.PEDERSEN_ROW_LANES
    want_s = {lanes * G: lanes, lanes * G + 1: lanes + 1, (lanes + 1) * G + 1: lanes + 2, cap: -(-cap // G)}
    assert max(want_s) == cap and want_s[cap] > 8 * lanes
    for cols, S in want_s.items():
        p = plan_of(prog, curve, cols)
        assert p == model(curve, cols), (curve, cols)
        assert p["S"] == S and (p["S"] > lanes) == (cols > lanes * G), (curve, cols)
        assert (p["S"] - 1) * p["g"] < cols <= p["S"] * p["g"] <= p["S"] * p["G"], (curve, cols)
        assert p["g"] * p["W"] <= p["max_entries"] and p["lds_bytes"] <= p["lds_max"], (curve, cols)


def test_every_column_count_near_the_slice_boundaries_is_covered(prog):
    """cols around every multiple of G up to 6 G (where balancing changes g), by the model the program was just shown to equal"""
    G = plan_of(prog, 0, 1)["G"]
    for cols in sorted({k * G + d for k in range(1, 7) for d in (-1, 0, 1)}):
        m = model(0, cols)
        assert (m["S"] - 1) * m["g"] < cols <= m["S"] * m["g"] and m["g"] <= m["G"], cols
