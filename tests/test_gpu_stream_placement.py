"""The order in which a context creates its streams (csrc/stream_place.hpp: rotated over the hardware queues when 1, 2 or 4 of them
serve the process, lane by lane otherwise) decides where a proof's packets queue, never what a proof is: a pipelined batch that turns
the lanes more than twice returns, limb for limb and flag for flag, the proofs of blocking calls.

One child process per setting (the runtime reads GPU_MAX_HW_QUEUES when it starts, a context latches ZKP_LANES / ZKP_GRAPH when it is
created).  A child that times out or dies fails the test; nothing is retried."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import random, sys
import numpy as np
from ckb_zkp_amd import codec, groth16
from ckb_zkp_amd.api import Context
from ckb_zkp_amd.circuits import mimc_chain_instance, samples_for_domain
n = int(sys.argv[1])
TOXIC = dict(alpha=11, beta=13, gamma=17, delta=19, tau=23)
ctx = Context(0)
inst = mimc_chain_instance("bn254", samples_for_domain(10))
params = groth16.generate_parameters(ctx, "bn254", inst, **TOXIC)
pk = groth16.ProvingKey(ctx, params, inst)
assert pk.domain_size == 1 << 10
c = params.curve
z = codec.fr_to_mont(inst.z, c).reshape(-1, 4)
zd = ctx.to_device(z)
rnd = random.Random(31)
rs = codec.fr_to_mont([rnd.randrange(c.r) for _ in range(n)], c)
ss = codec.fr_to_mont([rnd.randrange(c.r) for _ in range(n)], c)
assert len({(bytes(rs[i]), bytes(ss[i])) for i in range(n)}) == n
outs, infs = pk.prove_batch_raw([zd] * n, rs, ss)
print("BATCH", outs.tobytes().hex(), infs.tobytes().hex())
one = [pk.prove_raw(zd, rs[i], ss[i], z_on_device=True) for i in range(n)]
print("SINGLE", np.stack([o for o, _ in one]).tobytes().hex(), np.stack([f for _, f in one]).tobytes().hex())
ctx.dev_free(zd)
pk.free()
ctx.close()
'''


def _batch_and_single(n, **env_extra):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
    for name in ("ZKP_LANES", "ZKP_GRAPH"):
        if name not in env_extra:
            env.pop(name, None)
    out = subprocess.run([sys.executable, "-c", _CHILD, str(n)], env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {l.split()[0]: l.split()[1:] for l in out.stdout.splitlines() if l.startswith(("BATCH", "SINGLE"))}
    assert set(got) == {"BATCH", "SINGLE"}, out.stdout[-500:]
    return got


# two full turns of 8 lanes plus a remainder; with 3 lanes six turns and a remainder
@pytest.mark.parametrize("env", [dict(GPU_MAX_HW_QUEUES="4"), dict(GPU_MAX_HW_QUEUES="4", ZKP_LANES="3"), dict(GPU_MAX_HW_QUEUES="16")],
                         ids=["q4-lanes8", "q4-lanes3", "q16-lanes8"])
def test_pipelined_batch_equals_blocking_proofs(env):
    n = 20
    got = _batch_and_single(n, **env)
    proofs, flags = got["BATCH"]
    assert len(flags) == 2 * 3 * n and len(proofs) % n == 0 and len(proofs) >= 2 * 8 * 8 * n
    assert len({proofs[i * len(proofs) // n:(i + 1) * len(proofs) // n] for i in range(n)}) == n     # distinct (r, s): distinct proofs
    assert got["BATCH"] == got["SINGLE"]


def test_graph_replay_on_rotated_streams_equals_blocking_proofs():
    """ZKP_GRAPH=1 captures a proof from the lane's main stream and replays it from the third proof of a lane on: 8 proofs on 2 lanes"""
    got = _batch_and_single(8, GPU_MAX_HW_QUEUES="4", ZKP_GRAPH="1", ZKP_LANES="2")
    assert got["BATCH"] == got["SINGLE"]
