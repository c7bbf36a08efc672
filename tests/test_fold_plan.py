"""CPU: the host-side plan of the C fold of a Groth16 key (ckb_zkp_amd/csrc/groth16_fold_plan.hpp, used by groth16_key.hip's
fold_c_into_l).  tests/c/fold_plan.cpp includes that header alone and compares fold_heavy_cut with its definition (the candidates
"all columns above 1000 heavy" and "the k costliest heavy", 150 per heavy column, ties to "all heavy" and then to the smallest k)
over every cost vector of up to 5 entries from {0, 1, 999, 1000, 1001, 1150, 1151, 38000, 50000} and over 4000 random vectors of up
to 400 entries, checks the cases its comment names (12 columns of 38 000 all heavy, 3000 columns of 50 000 none, a fixed threshold
returned as given), and compares fold_column_costs and fold_build_csc with a brute-force transpose of random CSR matrices of up
to 12 rows x 10 variables with coefficients one, minus one and general: light columns, heavy lists, the prefix sum, a column index
>= nz refused; no row, no variable, no entry, every column heavy and none heavy among them."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
SRC = ROOT / "tests" / "c" / "fold_plan.cpp"
OUT = ROOT / "tests" / "c" / "build" / "fold_plan"


def test_the_fold_plan_agrees_with_its_definitions():
    OUT.parent.mkdir(parents=True, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{CSRC}", str(SRC), "-o", str(OUT)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(OUT)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[1]) > (9 ** 6 - 1) // 8 + 4000 + 3000
