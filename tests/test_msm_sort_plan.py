"""CPU: the geometry of the MSM bucket sort and of the task schedule (ckb_zkp_amd/csrc/msm_sort_plan.hpp, used by msm.hip).
tests/c/sort_plan.cpp includes that header alone and prints the plan of one shape per run; here every plan is compared with the
integer model in tests/msm_plan_ref.py (written from the host code that sized the sort before the header existed) and checked
against what the kernels rely on: at most 2^13 level-1 bins and 2^13 keys per bin (the LDS counters), at most 1536 tiles that are
multiples of 256 scalars, LDS sizes a CDNA4 compute unit has, and a schedule whose arrays neither overlap nor leave the buffer."""
import os
import subprocess
from pathlib import Path

import pytest

from tests import msm_plan_ref as M

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
SRC = ROOT / "tests" / "c" / "sort_plan.cpp"
OUT = ROOT / "tests" / "c" / "build" / "sort_plan"
LDS_PER_CU = 160 * 1024

NS = [1, 255, 2048, 2049, 4609, 1 << 20, 3 * (1 << 20) + 7, 1 << 24]
WS = [2, 13, 22, 32, 128]
KBITS = [3, 9, 13, 14, 19, 26]
FORCED_H1 = [0, 1, 13, 20]


@pytest.fixture(scope="module")
def prog():
    OUT.parent.mkdir(parents=True, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{CSRC}", str(SRC), "-o", str(OUT)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(OUT)


def plan_of(prog, n, W, sets, kbits, h1, staged, cap):
    r = subprocess.run([prog, *map(str, (n, W, sets, kbits, h1, int(staged), cap))], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (n, W, sets, kbits, h1, staged, cap, r.stdout, r.stderr)
    return {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}


def check_shape(prog, n, W, sets, kbits, h1, staged, cap):
    shape = (n, W, sets, kbits, h1, staged, cap)
    got = plan_of(prog, *shape)
    want = M.sort_plan(n, W, sets, kbits, h1, staged)
    if want is None:
        assert got == {"ok": 0}, shape
        return False
    nb, E = 1 << kbits, n * W * sets
    want.update(M.sched_layout(nb, E, cap), ok=1)
    assert got == want, shape
    p = got
    assert p["H1"] <= 13 and p["LB"] <= 13 and p["H1"] + p["LB"] == kbits, shape
    assert p["nblocks"] <= 1536 and p["tile"] % 256 == 0 and p["nblocks"] * p["tile"] >= n, shape
    if p["staged_sub"]:
        assert p["staged_sub"] % 256 == 0 and p["staged_sub"] <= p["tile"], shape
    assert p["staged_lds"] < LDS_PER_CU and p["bin_lds"] < LDS_PER_CU, shape
    # the schedule: [start, end) of every array in bytes, in the order they lie
    mt = p["max_tasks"]
    assert mt >= nb + E // cap, shape                             # a bucket of len entries is ceil(len / cap) <= 1 + len / cap tasks
    regions = [(4 * p[name], 4 * (p[name] + words)) for name, words in (("tcount", nb + 1), ("toff", nb + 1), ("task_start", mt),
               ("task_len", mt), ("task_dst", mt), ("long_list", mt), ("tmeta", M.TM_WORDS))] + [(p["desc_bytes"], p["desc_bytes"] + 16 * mt)]
    assert p["desc_bytes"] % 16 == 0, shape
    assert regions[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(regions, regions[1:])), shape
    assert regions[-1][1] <= 4 * p["words"], shape
    return True


@pytest.mark.parametrize("n", NS)
def test_plan_matches_the_model_and_keeps_its_bounds(prog, n):
    accepted = 0
    for W in WS:
        for sets in (1, 2):
            for kbits in KBITS:
                for h1 in FORCED_H1:
                    for staged in (True, False):
                        accepted += check_shape(prog, n, W, sets, kbits, h1, staged, 128)
    assert accepted == len(WS) * 2 * len(KBITS) * len(FORCED_H1) * 2        # one and two vectors always find a level-1 bit


def test_a_bin_that_would_straddle_two_vectors_is_refused(prog):
    # four vectors need two level-1 bits: one forced bit, or a one-bit bucket id, cannot separate them
    assert not check_shape(prog, 4609, 13, 4, 9, 1, True, 128)
    assert not check_shape(prog, 4609, 13, 4, 1, 0, True, 128)
    assert check_shape(prog, 4609, 13, 4, 9, 2, True, 128)


@pytest.mark.parametrize("cap", [4, 37])
def test_schedule_with_short_tasks(prog, cap):
    for n in NS:
        for sets in (1, 2):
            for kbits in KBITS:
                assert check_shape(prog, n, 13, sets, kbits, 0, True, cap)
