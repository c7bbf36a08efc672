"""CPU: where the levels of the bucket-reduction pyramid live when one kernel chain reduces several bucket sets
(ckb_zkp_amd/csrc/msm_pyramid.hpp, used by msm.hip).  tests/c/pyramid_layout.cpp includes that header alone and checks, for one
shape per run, that no two (set, level) regions overlap, that everything stays inside the bucket buffer of 2 * sets * nb points,
that one set gives the plain layout, and that the levels of the fused top sit where pair_top_body writes them."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
SRC = ROOT / "tests" / "c" / "pyramid_layout.cpp"
OUT = ROOT / "tests" / "c" / "build" / "pyramid_layout"


@pytest.fixture(scope="module")
def prog():
    OUT.parent.mkdir(parents=True, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{CSRC}", str(SRC), "-o", str(OUT)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(OUT)


# buckets per set of the fused-proof tests (2^6 .. 2^14 domains: c = 6, 9, 11, 13, 14), of the flagship (c = 20) and the smallest
SHAPES = [(1 << (c - 1), top_max, chunk) for c in (4, 6, 9, 11, 13, 14, 20) for top_max, chunk in ((2048, 4096), (2048, 1024), (2, 1024), (512, 4096))]


@pytest.mark.parametrize("sets", [1, 2, 4])
def test_sets_never_overlap(prog, sets):
    for nb_set, top_max, chunk in SHAPES:
        r = subprocess.run([prog, str(nb_set), str(sets), str(top_max), str(chunk), "1"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.startswith("ok"), (nb_set, sets, top_max, chunk, r.stdout)
        l_top, end = [int(x.split("=")[1]) for x in r.stdout.split()[1:]]
        # the top starts where a set holds top_max entries, or at the buckets themselves when there are fewer
        assert nb_set >> l_top == min(nb_set, top_max)
        assert end == 2 * sets * nb_set


def test_without_a_fused_top_one_set_is_the_plain_layout(prog):
    for nb_set, top_max, chunk in SHAPES:
        r = subprocess.run([prog, str(nb_set), "1", str(top_max), str(chunk), "0"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stdout.split()[:2] == ["ok", "l_top=-1"], (nb_set, r.stdout)
        assert int(r.stdout.split()[2].split("=")[1]) == 2 * nb_set - 1
