"""Circuits, assignments and transcript stand-ins shared by the Hyrax tests (tests/test_hyrax_ref.py, tests/test_gpu_hyrax.py)."""
import json
from pathlib import Path

from tests.gkr_cases import callbacks as gkr_callbacks, rand_fr

GOLDEN = Path(__file__).resolve().parent / "golden" / "hyrax_mini.json"


def load_golden():
    """{"mini": ..., "test": ...}: curve, layers (lists of (op, left, right)), inputs / witnesses (one list per copy), num_inputs,
    num_aux and pins (the round polynomials under `callbacks`, output points from `points`)"""
    d = json.loads(GOLDEN.read_text())
    out = {}
    for name in ("mini", "test"):
        e = d[name]
        out[name] = dict(curve=e["curve"], num_inputs=e["num_inputs"], num_aux=e["num_aux"],
                         layers=[[tuple(g) for g in layer] for layer in e["layers"]],
                         inputs=[[int(v) for v in row] for row in e["inputs"]],
                         witnesses=[[int(v) for v in row] for row in e["witnesses"]],
                         pins=[[[int(v) for v in poly] for poly in layer] for layer in e["pins"]])
    return out


def assignments(case, n, r, seed):
    """n copies for a golden circuit: the golden copies first, seeded values after them"""
    k_in, k_aux = len(case["inputs"][0]), len(case["witnesses"][0])
    inputs = [list(v) for v in case["inputs"][:n]]
    witnesses = [list(v) for v in case["witnesses"][:n]]
    for t in range(len(inputs), n):
        inputs.append(rand_fr(r, k_in, seed + 2 * t))
        witnesses.append(rand_fr(r, k_aux, seed + 2 * t + 1))
    return inputs, witnesses


def points(r, log_g, log_n, seed):
    """the output points (q, q') that eval_outputs would draw"""
    v = rand_fr(r, log_g + log_n, seed)
    return v[:log_g], v[log_g:]


def callbacks(r, tag=b"hyrax"):
    """(next_round, next_u): the hash chain of tests/gkr_cases.callbacks"""
    next_round, _, next_pair = gkr_callbacks(r, tag)
    return next_round, next_pair
