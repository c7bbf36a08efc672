"""GPU: bench.py as the driver runs it.  A plain run prints the headline line and measures nothing else; --full adds its
blocks and checks; both prove the same seeded inputs, so the proofs they dump are the same."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--log-n", "12"]


def _bench(args, detail, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT, ZKP_BENCH_DETAIL=str(detail))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                         timeout=timeout, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only_and_full_run_proves_the_same(tmp_path):
    plain = _bench(BASE + ["--dump-outputs", str(tmp_path / "plain")], tmp_path / "plain_detail.json")
    assert plain["metric"] == "Groth16 proofs/sec (2^12 domain, bn254)" and plain["unit"] == "proofs/s"
    assert plain["higher_is_better"] is True and plain["dtype"].startswith("u32 limbs")
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and (plain["steps"], plain["warmup"]) == (3, 2)
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["detail"] is None
    assert "msm_g1" not in plain and "summary" not in plain
    assert not (tmp_path / "plain_detail.json").exists()

    full = _bench(BASE + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")], tmp_path / "full_detail.json")
    assert full["metric"] == plain["metric"] and full["roofline"]["frac"] > 0 and full["msm_g1"]["mops"] > 0
    record = json.load(open(tmp_path / "full_detail.json"))
    assert record["latency"]["ms_per_proof"] > 0 and record["valu_roof"]["g1_accumulate"]["frac"] > 0

    names = sorted(p.name for p in (tmp_path / "plain").glob("*.npy"))
    assert names == ["proof_a.npy", "proof_b.npy", "proof_c.npy", "proof_infinity.npy"]
    assert names == sorted(p.name for p in (tmp_path / "full").glob("*.npy"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)), n
