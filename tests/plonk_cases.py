"""Circuits shared by the PLONK tests (tests/test_plonk_ref.py, tests/test_gpu_plonk.py).  Every builder drives a composer through
the method names that tests/plonk_ref.py's RefComposer and ckb_zkp_amd/plonk.py's Composer share, so one circuit feeds both."""
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "plonk_mini.json"
KS = [1, 7, 13, 17]                                                  # plonk/src/lib.rs:309-316
MINI_CHALLENGES = {"beta": 0x1234567890ABCDEF1122334455667788, "gamma": 0x0FEDCBA9876543211234, "alpha": 0x5DEECE66D0123456789ABCDEF}


def mini_circuit(cs):
    """plonk/src/lib.rs:318-359: 1 + 2 = 3, 1 + 3 = 4, 2 * 2 = 4, 2 * (1 * 2) + 2 = 6, six == 6.  5 gates, n = 8."""
    one, two, three, four, six = (cs.alloc_and_assign(v) for v in (1, 2, 3, 4, 6))
    cs.create_add_gate((one, 1), (two, 1), three, None, 0, 0)
    cs.create_add_gate((one, 1), (three, 1), four, None, 0, 0)
    cs.create_mul_gate(two, two, four, None, 1, 0, 0)
    cs.create_mul_gate(one, two, six, None, 2, 2, 0)
    cs.constrain_to_constant(six, 6, 0)
    return cs


def random_circuit(cs, gates, seed):
    """`gates` satisfied gates of every kind over variables that are reused (copy cycles of every length), with aux wires, constants
    and public inputs"""
    rng = np.random.default_rng(seed)
    r = cs.r
    big = lambda: int.from_bytes(rng.bytes(40), "little") % r          # noqa: E731
    vals = {}

    def alloc(v):
        var = cs.alloc_and_assign(v)
        vals[var] = v % r
        return var

    pool = [alloc(big()) for _ in range(4)] + [alloc(0), alloc(r - 1)]
    while cs.size() < gates:
        kind = int(rng.integers(0, 10))
        l, rr = (pool[int(i)] for i in rng.integers(0, len(pool), 2))
        aux = (pool[int(rng.integers(0, len(pool)))], big()) if rng.random() < 0.3 else None
        a0 = vals[aux[0]] * aux[1] if aux else 0
        if kind < 4:                                                 # a l + b r + aux + q_c + pi = o
            a, b, qc, pi = big(), big(), big(), (big() if rng.random() < 0.2 else 0)
            o = alloc(a * vals[l] + b * vals[rr] + a0 + qc + pi)
            cs.create_add_gate((l, a), (rr, b), o, aux, qc, pi)
        elif kind < 8:                                               # q_m l r + aux + q_c + pi = o
            qm, qc, pi = big(), big(), (big() if rng.random() < 0.2 else 0)
            o = alloc(qm * vals[l] * vals[rr] + a0 + qc + pi)
            cs.create_mul_gate(l, rr, o, aux, qm, qc, pi)
        elif kind == 8:
            o = alloc(vals[l])
            cs.assert_equal(l, o)
        else:
            pi = big() if rng.random() < 0.5 else 0
            cs.constrain_to_constant(l, vals[l] - pi, pi)
            continue
        pool.append(o)
        if len(pool) > 24:
            pool.pop(int(rng.integers(0, len(pool))))
    return cs


def rand_fr(r, n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % r for _ in range(n)]


def challenges(r, seed):
    b, g, a = rand_fr(r, 3, 7000 + seed)
    return b, g, a


def load_golden():
    d = json.loads(GOLDEN.read_text())
    for k, v in d.items():
        if isinstance(v, list):
            d[k] = [int(x) for x in v]
    for k in MINI_CHALLENGES:
        d[k] = int(d[k])
    return d


def make_golden():
    """the content of tests/golden/plonk_mini.json: tests/plonk_ref.py on BLS12-381"""
    from tests import plonk_ref as ref
    cs = mini_circuit(ref.RefComposer("bls12_381"))
    ix = ref.RefIndex(cs, KS)
    w = cs.synthesize()
    out = ref.prove_rounds(ix, w, cs.public_inputs(), MINI_CHALLENGES["beta"], MINI_CHALLENGES["gamma"], MINI_CHALLENGES["alpha"])
    assert out["closes"]
    d = {"curve": "bls12_381", "n": ix.n, "ks": KS}
    d.update({k: str(v) for k, v in MINI_CHALLENGES.items()})
    for name in ref.Q_NAMES + ref.S_NAMES:
        d[name] = [str(v) for v in ix.sel[name]]
    for j in range(4):
        d[f"witness_{j}"] = [str(v) for v in w[j]]
    d["pi"] = [str(v) for v in cs.public_inputs()]
    for name in ("z", "t_0", "t_1", "t_2", "t_3"):
        d[name] = [str(v) for v in out[name]]
    return d


if __name__ == "__main__":
    GOLDEN.write_text(json.dumps(make_golden(), indent=1) + "\n")
