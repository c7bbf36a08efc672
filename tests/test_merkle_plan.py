"""CPU: the launch plan of zkp_fr_merkle_tree_dev (ckb_zkp_amd/csrc/fr_hash.hpp merkle_plan, used by fr_hash.hip).
tests/c/merkle_plan.cpp includes that header alone and prints the plan of every n of a range; here every plan is checked against
what the kernels rely on: the launches partition the inner nodes [0, n - 1), the children of a launch's nodes are leaves or nodes
of earlier launches (of deeper depths inside the tail), a depth launch covers exactly one depth, the tail fits its one workgroup,
and the launch count is max(0, D - 8) + 1 with D = depth(n - 2); n = 1 launches nothing.  ckb_zkp_amd.merkle.launch_plan restates
the plan in Python and must agree."""
import os
import subprocess
from pathlib import Path

import pytest

from ckb_zkp_amd import hashes, merkle

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
SRC = ROOT / "tests" / "c" / "merkle_plan.cpp"
OUT = ROOT / "tests" / "c" / "build" / "merkle_plan"
RANGES = [(1, 3000), ((1 << 20) - 1, (1 << 20) + 1)]


@pytest.fixture(scope="module")
def plans():
    OUT.parent.mkdir(parents=True, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{CSRC}", str(SRC), "-o", str(OUT)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for lo, hi in RANGES:
        r = subprocess.run([str(OUT), str(lo), str(hi)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        for line in r.stdout.splitlines():
            n, tail_nodes, *launches = line.split()
            assert int(tail_nodes) == hashes.HASH_TAIL_NODES
            out[int(n)] = [(int(a), int(b), c == "1") for a, b, c in (l.split(":") for l in launches)]
    return out


def test_every_n_is_planned(plans):
    assert sorted(plans) == list(range(1, 3001)) + [(1 << 20) - 1, 1 << 20, (1 << 20) + 1]
    assert plans[1] == []


def test_ranges_partition_the_inner_nodes_and_children_come_first(plans):
    tail_span = 2 * hashes.HASH_TAIL_NODES - 1
    for n, plan in plans.items():
        if n == 1:
            continue
        inner = n - 1
        done_from = inner                                  # nodes [done_from, 2 n - 1) exist: the leaves, then what was launched
        for k, (lo, hi, tail) in enumerate(plan):
            assert lo < hi == done_from, (n, k)           # adjacent to what exists, downwards: a partition in the end
            assert tail == (k == len(plan) - 1), (n, k)
            if tail:
                assert lo == 0 and hi <= tail_span
                # inside the tail the depths run from the deepest up; depth d has at most HASH_TAIL_NODES nodes
                for d in range(merkle.depth(hi - 1), -1, -1):
                    dlo, dhi = (1 << d) - 1, min((2 << d) - 1, hi)
                    assert 0 < dhi - dlo <= hashes.HASH_TAIL_NODES
                    assert 2 * dlo + 1 >= dhi and 2 * (dhi - 1) + 2 <= 2 * n - 2          # children: below this depth, inside the tree
            else:
                assert merkle.depth(lo) == merkle.depth(hi - 1) >= hashes.HASH_TAIL_DEPTHS      # one depth
                assert lo == (1 << merkle.depth(lo)) - 1
                assert 2 * lo + 1 >= hi and 2 * (hi - 1) + 2 <= 2 * n - 2                 # children exist already
            done_from = lo
        assert done_from == 0, n


def test_launch_count_is_the_formula_and_python_agrees(plans):
    for n, plan in plans.items():
        if n == 1:
            assert merkle.launch_plan(1) == []
            continue
        D = merkle.depth(n - 2)
        assert len(plan) == max(0, D - 8) + 1, n
        assert plan == merkle.launch_plan(n), n
    assert len(plans[513]) == 2 and plans[513][0] == (511, 512, False)                  # a depth launch of one node
    assert [l[:2] for l in plans[1025]] == [(1023, 1024), (511, 1023), (0, 511)]       # two depth launches plus the tail
    assert len(plans[512]) == 1 and len(plans[1 << 20]) == 12
