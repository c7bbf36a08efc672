"""CPU: the table of internal A/B switches (ckb_zkp_amd/csrc/tune.hpp).

tests/c/tune_table.cpp includes that header and nothing else of the library, sets the environment it is given and prints what a
context created at that moment would latch.  Every expected value below was written down from the code that read the variable
before the table existed (the `static const ... getenv` lines of ntt / msm / msm_acc / groth16 / marlin), not taken from the header.

ZKP_C_DRIVER_FLAGS="-fsanitize=address,undefined" builds the program sanitized, as for tests/c/abi_driver.c."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
SRC = ROOT / "tests" / "c" / "tune_table.cpp"
OUT = ROOT / "tests" / "c" / "build" / "tune_table"

# default on: off only by a value that reads as 0 | default off: on by any value that reads as non-zero
ON = ["ZKP_NTT_V2", "ZKP_NTT_FULL", "ZKP_NTT_FUSE", "ZKP_SHARE_B_SORT", "ZKP_SHARE_AL_SORT", "ZKP_SHARE_L1", "ZKP_CHAIN_LH",
      "ZKP_WM_FIRST", "ZKP_L_OWN_STREAM", "ZKP_G2_EARLY", "ZKP_MSM_WIDEN", "ZKP_MSM_BALANCED", "ZKP_SORT_STAGED",
      "ZKP_PAIR_TOP_FUSE_SEG", "ZKP_PAIR_TOP", "ZKP_MARLIN_EARLY", "ZKP_MARLIN_HOST_AFFINE"]
OFF = ["ZKP_B_WINDOW", "ZKP_NTT_BATCH", "ZKP_SINGLE_STREAM", "ZKP_GRAPH", "ZKP_TIMELINE", "ZKP_MEMSET_BUCKETS",
       "ZKP_DEBUG_FORCE_REDO", "ZKP_MARLIN_EARLY_FFT", "ZKP_MARLIN_EARLY_EVAL"]
# -1: "unset" where the old code told an unset variable from every value it could hold; 0 where 0 already meant "no override"
INTS = {"ZKP_NTT_SMAX": 9, "ZKP_B_WINDOW_BITS": -1, "ZKP_B_TASK_CAP": -1, "ZKP_LATENCY_PLAN": -1, "ZKP_DEBUG_SKIP_K8_MASK": 0,
        "ZKP_TABLE_K": 0, "ZKP_TASK_CAP": 0, "ZKP_TASK_CAP_G2": 0, "ZKP_MSM_CHUNK_FIRST": 2, "ZKP_SORT_H1": 0,
        "ZKP_SORT_NT_HIST": 1024, "ZKP_SORT_NT_SCATTER": 512, "ZKP_TASK_NT": 1024, "ZKP_DEBUG_MSM": 0, "ZKP_PAIR_TOP_MAX": 2048,
        "ZKP_MSM_VAR_C": 0, "ZKP_ACC_LDS_BYTES": 0, "ZKP_G2_ACC_OCC": 2, "ZKP_G1_ACC_OCC": 3, "ZKP_G1_ACC_WAVES": 0}
DEFAULTS = {**{k: 1 for k in ON}, **{k: 0 for k in OFF}, **INTS}

# (environment, what differs from DEFAULTS): below / inside / above every range, and every value that selects something
CASES = [
    ({"ZKP_NTT_SMAX": "3"}, {"ZKP_NTT_SMAX": 4}),
    ({"ZKP_NTT_SMAX": "7"}, {"ZKP_NTT_SMAX": 7}),
    ({"ZKP_NTT_SMAX": "12"}, {"ZKP_NTT_SMAX": 10}),
    # three instantiations per kernel: >= 1024, >= 512, else 256
    ({"ZKP_TASK_NT": "100", "ZKP_SORT_NT_HIST": "0", "ZKP_SORT_NT_SCATTER": "511"},
     {"ZKP_TASK_NT": 256, "ZKP_SORT_NT_HIST": 256, "ZKP_SORT_NT_SCATTER": 256}),
    ({"ZKP_TASK_NT": "512", "ZKP_SORT_NT_HIST": "600", "ZKP_SORT_NT_SCATTER": "1023"},
     {"ZKP_TASK_NT": 512, "ZKP_SORT_NT_HIST": 512, "ZKP_SORT_NT_SCATTER": 512}),
    ({"ZKP_TASK_NT": "4096", "ZKP_SORT_NT_HIST": "1024", "ZKP_SORT_NT_SCATTER": "2000"},
     {"ZKP_TASK_NT": 1024, "ZKP_SORT_NT_HIST": 1024, "ZKP_SORT_NT_SCATTER": 1024}),
    ({"ZKP_MSM_VAR_C": "3"}, {}),
    ({"ZKP_MSM_VAR_C": "4"}, {"ZKP_MSM_VAR_C": 4}),
    ({"ZKP_MSM_VAR_C": "8"}, {"ZKP_MSM_VAR_C": 8}),
    ({"ZKP_MSM_VAR_C": "16"}, {"ZKP_MSM_VAR_C": 16}),
    ({"ZKP_MSM_VAR_C": "32"}, {}),
    # >= 4, at most MSM_TASK_CAP = 128; G2 bases follow unless ZKP_TASK_CAP_G2 is SET (a set value below 4 overrides nothing)
    ({"ZKP_TASK_CAP": "3"}, {}),
    ({"ZKP_TASK_CAP": "64"}, {"ZKP_TASK_CAP": 64, "ZKP_TASK_CAP_G2": 64}),
    ({"ZKP_TASK_CAP": "1000"}, {"ZKP_TASK_CAP": 128, "ZKP_TASK_CAP_G2": 128}),
    ({"ZKP_TASK_CAP": "64", "ZKP_TASK_CAP_G2": "2"}, {"ZKP_TASK_CAP": 64, "ZKP_TASK_CAP_G2": 0}),
    ({"ZKP_TASK_CAP": "64", "ZKP_TASK_CAP_G2": "32"}, {"ZKP_TASK_CAP": 64, "ZKP_TASK_CAP_G2": 32}),
    ({"ZKP_TASK_CAP_G2": "500"}, {"ZKP_TASK_CAP_G2": 128}),
    ({"ZKP_MSM_CHUNK_FIRST": "0"}, {"ZKP_MSM_CHUNK_FIRST": 1}),
    ({"ZKP_MSM_CHUNK_FIRST": "-5"}, {"ZKP_MSM_CHUNK_FIRST": 1}),
    ({"ZKP_MSM_CHUNK_FIRST": "3"}, {"ZKP_MSM_CHUNK_FIRST": 3}),
    # set: the group size is forced (0 and 1: groups of one), rounded up to a power of two, at most 2^6
    ({"ZKP_TABLE_K": "0"}, {"ZKP_TABLE_K": 1}),
    ({"ZKP_TABLE_K": "1"}, {"ZKP_TABLE_K": 1}),
    ({"ZKP_TABLE_K": "2"}, {"ZKP_TABLE_K": 2}),
    ({"ZKP_TABLE_K": "3"}, {"ZKP_TABLE_K": 4}),
    ({"ZKP_TABLE_K": "64"}, {"ZKP_TABLE_K": 64}),
    ({"ZKP_TABLE_K": "100"}, {"ZKP_TABLE_K": 64}),
    # below 2: the default; else rounded DOWN to a power of two
    ({"ZKP_PAIR_TOP_MAX": "1"}, {}),
    ({"ZKP_PAIR_TOP_MAX": "1000"}, {"ZKP_PAIR_TOP_MAX": 512}),
    ({"ZKP_PAIR_TOP_MAX": "2048"}, {}),
    ({"ZKP_PAIR_TOP_MAX": "5000"}, {"ZKP_PAIR_TOP_MAX": 4096}),
    ({"ZKP_B_WINDOW_BITS": "0", "ZKP_B_TASK_CAP": "0"}, {"ZKP_B_WINDOW_BITS": 0, "ZKP_B_TASK_CAP": 0}),
    ({"ZKP_B_WINDOW_BITS": "17", "ZKP_B_TASK_CAP": "48"}, {"ZKP_B_WINDOW_BITS": 17, "ZKP_B_TASK_CAP": 48}),
    ({"ZKP_LATENCY_PLAN": "0"}, {"ZKP_LATENCY_PLAN": 0}),
    ({"ZKP_LATENCY_PLAN": "1"}, {"ZKP_LATENCY_PLAN": 1}),
    ({"ZKP_DEBUG_SKIP_K8_MASK": "0x11"}, {"ZKP_DEBUG_SKIP_K8_MASK": 17}),
    ({"ZKP_SORT_H1": "12", "ZKP_ACC_LDS_BYTES": "4096", "ZKP_G2_ACC_OCC": "3", "ZKP_G1_ACC_OCC": "4", "ZKP_G1_ACC_WAVES": "3",
      "ZKP_DEBUG_MSM": "2"},
     {"ZKP_SORT_H1": 12, "ZKP_ACC_LDS_BYTES": 4096, "ZKP_G2_ACC_OCC": 3, "ZKP_G1_ACC_OCC": 4, "ZKP_G1_ACC_WAVES": 3,
      "ZKP_DEBUG_MSM": 2}),
]


@pytest.fixture(scope="module")
def tune_table():
    OUT.parent.mkdir(exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{CSRC}", str(SRC), "-o", str(OUT)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(env):
        out = subprocess.run([str(OUT)] + [f"{k}={v}" for k, v in env.items()], capture_output=True, text=True, timeout=60,
                             env=dict(os.environ, ZKP_NTT_SMAX="5", ZKP_GRAPH="1"))      # inherited settings must not leak in
        assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
        rows = [l.split("=") for l in out.stdout.splitlines()]
        assert len({k for k, _ in rows}) == len(rows)                                     # one line per switch
        return {k: int(v) for k, v in rows}
    return run


def test_every_switch_has_its_documented_default(tune_table):
    assert tune_table({}) == DEFAULTS


def test_flags_read_zero_as_off_and_non_zero_as_on(tune_table):
    flags = ON + OFF
    assert tune_table({k: "0" for k in flags}) == {**DEFAULTS, **{k: 0 for k in flags}}
    assert tune_table({k: "1" for k in flags}) == {**DEFAULTS, **{k: 1 for k in flags}}
    assert tune_table({k: "7" for k in OFF}) == {**DEFAULTS, **{k: 1 for k in OFF}}


@pytest.mark.parametrize("env,differs", CASES, ids=[",".join(f"{k[4:]}={v}" for k, v in e.items()) for e, _ in CASES])
def test_integers_are_clamped_as_before(tune_table, env, differs):
    assert tune_table(env) == {**DEFAULTS, **differs}


def header_rows():
    text = (CSRC / "tune.hpp").read_text()
    return re.findall(r'^\s*(FLAG|INT|MASK)\s*\(\s*(\w+)\s*,\s*"(ZKP_\w+)"\s*,\s*([^,]+),', text, flags=re.M)


def test_the_environment_is_read_in_the_table_only():
    """`getenv(` appears in tune.hpp and in the ZKP_DEBUG_GATHER block of msm_acc.hip (profiling builds), nowhere else; what still
    reads the environment at call time says so by name (env_str); no function-local static is initialised from it."""
    live = {"ZKP_DEBUG_MSM", "ZKP_DEBUG_RCCL_HANG"}
    latched_elsewhere = {"capi.hip"}                          # cfg_from_env, at context creation like the table
    for p in sorted(CSRC.iterdir()):
        if p.suffix not in (".hip", ".hpp", ".cpp", ".inc") or p.name == "tune.hpp":
            continue
        for no, line in enumerate(p.read_text().splitlines(), 1):
            where = f"{p.name}:{no}: {line.strip()}"
            if "getenv(" in line:
                assert p.name == "msm_acc.hip" and "ZKP_DEBUG_GATHER_MASK" in line, where
            for call in re.finditer(r'\benv_(?:str|num|flag)\(\s*("(\w+)")?', line):
                assert not re.search(r"\bstatic\b", line), where
                assert p.name in latched_elsewhere or call.group(2) in live, where


def test_design_md_lists_exactly_the_switches_of_the_header():
    rows = header_rows()
    assert {env for _, _, env, _ in rows} == set(DEFAULTS)                   # the header and this test know the same switches
    assert len({f for _, f, _, _ in rows}) == len(rows) == len(DEFAULTS)
    doc = re.findall(r"^\| `(ZKP_\w+)` \| ([^|]+) \|", (ROOT / "DESIGN.md").read_text(), flags=re.M)
    assert len(doc) == len({n for n, _ in doc})
    shown = {"ZKP_TASK_CAP_G2": "ZKP_TASK_CAP"}                                # its default is another switch's value
    assert {n: d.strip() for n, d in doc} == {k: shown.get(k, str(v)) for k, v in DEFAULTS.items()}
