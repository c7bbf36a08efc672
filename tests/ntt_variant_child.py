"""NTT variants, one fresh process per switch setting (tests/test_gpu_ntt_variants.py).

The switches of csrc/ntt.hip (ZKP_NTT_V2 / _FULL / _FUSE / _SMAX) and ZKP_NTT_BATCH of the witness map are latched by a context when
it is created (csrc/tune.hpp).  Every setting is still checked by a child of its own, so that a child that faults stops the
run (last paragraph) instead of taking the other settings' checks with it:

    python -m tests.ntt_variant_child '{"ntt": [log_n, ...], "witness": [k, ...]}'      (switches in the environment)

The child opens one Context(0), runs the checks of the spec on both scalar fields and prints one JSON line
{"checked": <int>, "mismatches": [[curve, what, log_n, op, first_bad_index], ...]}.  It does not assert: `run_variant` (the parent's
half, below) does, and also compares `checked` with the count it derives from the spec itself, so that a child that skipped work
cannot pass.

  ntt      every input of `inputs()` through all four ops of ctx.ntt == oracle/cpu's transform, word for word
  witness  pk.witness_map(z) of a matrices-only key of the 2^k MiMC chain == oracle/cpu's witness_map, word for word

A child that dies of a signal / an abort / a time limit / a GPU fault fails its test AND stops every later variant case before it
starts a process (`gpu_dead`): nothing more is launched on a device that has just faulted, and nothing is retried."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

CURVES = ("bn254", "bls12_381")
OPS = (0, 1, 2, 3)                       # fft, ifft, coset_fft, coset_ifft (zkp_ntt_op)
DEFAULT_SMAX = 9                         # NTT_SMAX of csrc/ntt.hip
UNIT_MAX_LOG = 14                        # unit vectors (and their closed form) for 2^1 .. 2^14
DENSE = ("uniform", "all_max", "alternating")
ILLEGAL_ACCESS = "illegal memory access"
FATAL_CODES = (124, 134, 137, 139)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

gpu_dead = None                          # set to a description by the first child that died; later variant cases fail at once


def _r(a, b):
    return list(range(a, b + 1))


# id, switches, `ntt` log_n, `witness` k
VARIANTS = [
    ("legacy", {"ZKP_NTT_V2": "0"}, _r(1, 14) + [17], [4, 9, 11]),
    ("twolevel", {"ZKP_NTT_FULL": "0"}, _r(0, 14) + [17, 19], [4, 9, 12]),
    ("legacy-twolevel", {"ZKP_NTT_V2": "0", "ZKP_NTT_FULL": "0"}, [3, 9, 11, 13], [11]),
    ("smax4", {"ZKP_NTT_SMAX": "4"}, _r(5, 17), [9, 10, 12, 13]),
    ("smax4-legacy", {"ZKP_NTT_SMAX": "4", "ZKP_NTT_V2": "0"}, _r(9, 13), [9]),
    ("smax4-twolevel", {"ZKP_NTT_SMAX": "4", "ZKP_NTT_FULL": "0"}, [9, 13], [9, 13]),
    ("smax7", {"ZKP_NTT_SMAX": "7"}, [8, 9, 15, 16, 18], [15]),
    ("smax10", {"ZKP_NTT_SMAX": "10"}, [10, 19], [10]),
    ("batch", {"ZKP_NTT_BATCH": "1"}, [], [5, 10, 12]),
    ("batch-smax4", {"ZKP_NTT_BATCH": "1", "ZKP_NTT_SMAX": "4"}, [], [9, 12, 13]),
    ("batch-twolevel", {"ZKP_NTT_BATCH": "1", "ZKP_NTT_FULL": "0", "ZKP_NTT_SMAX": "4"}, [], [9]),
    ("nofuse", {"ZKP_NTT_FUSE": "0"}, [], [4, 9, 12]),
]


# ------------------------------------------------------------------------------------------------ spec arithmetic (no GPU)
def smax_of(env) -> int:
    """ntt_smax of csrc/tune.hpp: ZKP_NTT_SMAX clamped to 4..10, default 9"""
    e = env.get("ZKP_NTT_SMAX")
    s = int(e) if e else DEFAULT_SMAX
    return min(max(s, 4), 10)


def plan(log_n: int, smax: int = DEFAULT_SMAX) -> list:
    """ntt_plan() of csrc/ntt.hip: radix bits per pass, the remainder on the first passes"""
    if log_n == 0:
        return []
    p = (log_n + smax - 1) // smax
    base, rem = divmod(log_n, p)
    return [base + (1 if i < rem else 0) for i in range(p)]


def unit_positions(log_n: int, smax: int = DEFAULT_SMAX) -> list:
    """j of the unit-vector inputs: 1, the last column of the first pass's first row, the first column of its second row, N - 1
    (rows of the first pass's tile are N / 2^S1 elements apart)"""
    if not 1 <= log_n <= UNIT_MAX_LOG:
        return []
    n = 1 << log_n
    rows = n >> plan(log_n, smax)[0]
    return sorted({j for j in (1, rows - 1, rows, n - 1) if 0 <= j < n})


def input_names(log_n: int, smax: int = DEFAULT_SMAX) -> list:
    return list(DENSE) + [f"unit{j}" for j in unit_positions(log_n, smax)]


def expected_checked(spec: dict, smax: int = DEFAULT_SMAX) -> int:
    """what a child that did all of `spec` reports: one per (curve, log_n, input, op) and one per (curve, k)"""
    ntt = sum(len(OPS) * len(input_names(lg, smax)) for lg in spec.get("ntt", []))
    return len(CURVES) * (ntt + len(spec.get("witness", [])))


# ------------------------------------------------------------------------------------------------ inputs (host, Montgomery residues)
def uniform_below_r(rng, n, c):
    """(n, 4) limbs of integers spread over [0, r): 192 random low bits, top limb uniform below r's top limb"""
    a = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
    a[:, 3] = rng.integers(0, c.r >> 192, size=n, dtype=np.uint64)
    return a


def _limbs(x: int) -> np.ndarray:
    return np.frombuffer(int(x).to_bytes(32, "little"), dtype="<u8").copy()


def make_input(curve, log_n: int, name: str) -> np.ndarray:
    """Every word pattern is a valid Montgomery residue (< r).  r - 1 is the largest one: all of them at once is the worst case of
    the unsaturated tile, whose values grow by 2p per stage without a reduction."""
    from ckb_zkp_amd.params import get_curve
    c = get_curve(curve)
    n = 1 << log_n
    top = _limbs(c.r - 1)
    if name == "uniform":
        x = uniform_below_r(np.random.default_rng(7000 + 100 * c.cid + log_n), n, c)
        x[0] = 0
        if n > 1:
            x[1] = top
        return x
    if name == "all_max":
        return np.tile(top, (n, 1))
    if name == "alternating":
        x = np.zeros((n, 4), dtype=np.uint64)
        x[0::2] = top
        return x
    assert name.startswith("unit")
    x = np.zeros((n, 4), dtype=np.uint64)
    x[int(name[4:])] = _limbs((1 << 256) % c.r)                     # Montgomery one
    return x


def inputs(curve, log_n: int, smax: int = DEFAULT_SMAX):
    for name in input_names(log_n, smax):
        yield name, make_input(curve, log_n, name)


def first_bad(got: np.ndarray, exp: np.ndarray) -> int:
    if got.shape != exp.shape:
        return -2
    bad = np.flatnonzero((got != exp).any(axis=1))
    return int(bad[0]) if len(bad) else -1


def witness_only_parameters(c, inst):
    """Parameters for a matrices-only key: the witness map reads the three matrices and nothing of the queries"""
    from ckb_zkp_amd.groth16 import Parameters
    g1, g2 = np.zeros(2 * c.fq_limbs, dtype=np.uint64), np.zeros(4 * c.fq_limbs, dtype=np.uint64)
    none1 = (np.zeros((0, 2 * c.fq_limbs), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    none2 = (np.zeros((0, 4 * c.fq_limbs), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    return Parameters(curve=c, num_inputs=inst.num_inputs, num_aux=inst.num_aux, num_constraints=inst.num_constraints(),
                      alpha_g1=g1, beta_g1=g1, beta_g2=g2, gamma_g2=g2, delta_g1=g1, delta_g2=g2, gamma_abc_g1=none1,
                      a_query=none1, b_g1_query=none1, b_g2_query=none2, h_query=none1, l_query=none1)


# ------------------------------------------------------------------------------------------------ the child's checks
def check_ntt(ctx, oracle, log_ns, smax: int, mismatches: list) -> int:
    from tests.util import OC
    checked = 0
    for curve in CURVES:
        for log_n in log_ns:
            for name, x in inputs(curve, log_n, smax):
                for op in OPS:
                    bad = first_bad(ctx.ntt(curve, x, op), oracle.ntt(OC[curve].cid, x, op, threads=8))
                    checked += 1
                    if bad != -1:
                        mismatches.append([curve, name, log_n, op, bad])
    return checked


def check_witness(ctx, oracle, ks, mismatches: list) -> int:
    from ckb_zkp_amd import codec, groth16
    from ckb_zkp_amd.circuits import mimc_chain_instance, samples_for_domain
    from ckb_zkp_amd.params import get_curve
    checked = 0
    for curve in CURVES:
        c = get_curve(curve)
        for k in ks:
            inst = mimc_chain_instance(curve, samples_for_domain(k))
            params = witness_only_parameters(c, inst)
            pk = groth16.ProvingKey(ctx, params, inst, matrices_only=True)
            try:
                z = codec.fr_to_mont(inst.z, c).reshape(-1, 4)
                bad = -3 if pk.domain_size != 1 << k else first_bad(pk.witness_map(z), oracle.witness_map(params, inst, z, threads=8))
            finally:
                pk.free()
            checked += 1
            if bad != -1:
                mismatches.append([curve, "witness", k, -1, bad])
    return checked


def run_spec(ctx, oracle, spec: dict, smax: int) -> dict:
    mismatches = []
    checked = check_ntt(ctx, oracle, spec.get("ntt", []), smax, mismatches)
    checked += check_witness(ctx, oracle, spec.get("witness", []), mismatches)
    return {"checked": checked, "mismatches": mismatches}


def main(argv) -> int:
    spec = json.loads(argv[1])
    from ckb_zkp_amd.api import Context
    from oracle import cpu_oracle
    with Context(0) as ctx:
        res = run_spec(ctx, cpu_oracle, spec, smax_of(os.environ))
    print(json.dumps(res), flush=True)
    return 0


# ------------------------------------------------------------------------------------------------ the parent's half
def child_died(returncode: int, output: str):
    """a description if the child ended with a signal, an abort / segmentation fault / time-limit status or a GPU fault, else None"""
    if returncode < 0:
        return f"signal {-returncode}"
    if returncode in FATAL_CODES:
        return f"exit status {returncode}"
    if ILLEGAL_ACCESS in output:
        return "HIP reported an illegal memory access"
    return None


def run_variant(switches: dict, spec: dict, argv=None, timeout: float = 300) -> dict:
    """One child for one switch setting; asserts everything the child does not.  argv: the child's command (tests of this
    function itself pass a stand-in)."""
    global gpu_dead
    assert gpu_dead is None, f"not started: an earlier NTT variant child died ({gpu_dead})"
    env = dict(os.environ, PYTHONPATH=ROOT, **switches)
    cmd = argv or [sys.executable, "-m", "tests.ntt_variant_child", json.dumps(spec)]
    try:
        out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        gpu_dead = f"{switches}: no answer within {timeout} s"
        raise AssertionError(f"child died: {gpu_dead}\n{str(e.stderr or '')[-2000:]}")
    died = child_died(out.returncode, out.stdout + out.stderr)
    if died:
        gpu_dead = f"{switches}: {died}"
        raise AssertionError(f"child died: {gpu_dead}\n{out.stderr[-2000:]}")
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-2000:]
    res = json.loads(lines[-1])
    assert res["mismatches"] == [], (switches, res["mismatches"][:8])
    assert res["checked"] == expected_checked(spec, smax_of(switches)), (switches, res["checked"])
    return res


if __name__ == "__main__":
    sys.exit(main(sys.argv))
