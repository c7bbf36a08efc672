"""Circuits and transcript stand-ins shared by the GKR tests (tests/test_gkr_ref.py, tests/test_gpu_gkr.py)."""
import hashlib
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "libra_mini.json"


def load_mini():
    """(curve, layers_raw, inputs, witnesses) of libra/tests/mini.rs"""
    d = json.loads(GOLDEN.read_text())
    layers = [[tuple(g) for g in layer] for layer in d["layers"]]
    return d["curve"], layers, [int(v) for v in d["inputs"]], [int(v) for v in d["witnesses"]]


def random_layers(widths, below, seed, hot=None):
    """layers_raw with widths[i] gates in layer i + 1 over `below` nodes of the input layer; every node index and both ops occur
    where the width allows.  hot = (layer, node, share): that share of the layer's gates read `node` on both wires."""
    rng = np.random.default_rng(seed)
    layers = []
    for i, w in enumerate(widths):
        op = rng.integers(0, 2, size=w)
        left, right = rng.integers(0, below, size=w), rng.integers(0, below, size=w)
        left[0], right[0] = below - 1, 0
        if w > 1:
            left[-1] = right[-1] = below - 1                       # left == right at the last node
            op[0], op[1] = 0, 1
        if hot and hot[0] == i:
            pick = rng.random(w) < hot[2]
            left[pick] = hot[1]
            right[rng.random(w) < hot[2]] = hot[1]
        layers.append([(int(o), int(a), int(b)) for o, a, b in zip(op, left, right)])
        below = w
    return layers


def rand_fr(r, n, seed):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes(40), "little") % r for _ in range(n)]


def callbacks(r, tag=b""):
    """deterministic stand-ins for the transcript: a counter plus whatever the reference would have absorbed.
    Returns (next_round, absorb_final, next_alpha_beta)."""
    state = {"n": 0, "seen": b""}

    def h(*parts):
        state["n"] += 1
        data = tag + state["n"].to_bytes(4, "little") + state["seen"] + b"".join(int(v).to_bytes(32, "little") for v in parts)
        state["seen"] = hashlib.sha256(data).digest()
        return int.from_bytes(state["seen"], "little") % r

    def absorb_final(values):
        h(*values)

    return (lambda coeffs: h(*coeffs)), absorb_final, (lambda: (h(1), h(2)))
