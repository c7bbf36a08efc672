"""MiMC, Poseidon and Rescue on the device (gadgets/src/hashes/{mimc,poseidon,rescue}.rs): resident parameters, batched blocks, the
`*_hash` chains and the mimc gadget's auxiliary assignment, over zkp_hash_params_* / zkp_fr_hash_* / zkp_fr_mimc_trace_dev.

Every constant is the caller's: Python integers in, a resident handle out.  Nothing here ships a table, and nothing is pinned to the
reference's literal constants; tests/hash_ref.py restates the permutations over Python integers.  Vectors on the device are
Montgomery Fr, 32 bytes each.  There is no CPU fallback."""
from __future__ import annotations

import numpy as np

from .circuits import MIMC_ROUNDS
from .codec import fr_mont, fr_to_mont
from .params import get_curve

KIND_MIMC, KIND_POSEIDON, KIND_RESCUE = 0, 1, 2            # zkp_hash_kind
HASH_WIDTH = 3                                            # ZKP_HASH_WIDTH, csrc/fr_hash.hpp
HASH_THREADS = 64
HASH_TAIL_NODES = 256
HASH_TAIL_DEPTHS = 9
HASH_RESCUE_WINDOW = 2
HASH_MAX_ROUNDS_MIMC = 512
HASH_MAX_ROUNDS_POSEIDON = 128
HASH_MAX_ROUNDS_RESCUE = 64
HASH_MAX_LOG_BLOCKS = 28
HASH_MAX_LOG_LEAVES = 27


def rescue_inv_alpha(curve, alpha: int) -> int:
    """alpha^-1 mod (r - 1): x -> x^alpha is then a permutation of Fr and this exponent undoes it"""
    return pow(alpha, -1, get_curve(curve).r - 1)


def poseidon_schedule(full_head: int, partial: int, full_tail: int) -> list:
    """full_head full rounds, `partial` partial rounds, full_tail full rounds -> one flag per round"""
    return [1] * full_head + [0] * partial + [1] * full_tail


def poseidon_reference_schedule(rounds: int, rf: int) -> list:
    """the schedule poseidon.rs:560 runs: round i is full unless i == rf / 2, so exactly one round is partial"""
    return [0 if i == rf // 2 else 1 for i in range(rounds)]


def bytes_to_elements(b: bytes, curve) -> list:
    """The chunking of the reference's `*_hash` (mimc.rs:65-76): 32-byte little-endian chunks, a last partial chunk zero-extended,
    a chunk that is no canonical element (>= r) mapped to 0."""
    r = get_curve(curve).r
    out = []
    for off in range(0, len(b), 32):
        v = int.from_bytes(b[off:off + 32], "little")
        out.append(v if v < r else 0)
    return out


class HashParams:
    """zkp_hash_params: the constants of one hash, resident on the device of `ctx`"""

    def __init__(self, ctx, curve, kind: int, rounds: int, handle: int):
        self.ctx, self.curve, self.kind, self.rounds, self.handle = ctx, get_curve(curve), kind, rounds, handle

    @classmethod
    def mimc(cls, ctx, curve, constants) -> "HashParams":
        c = get_curve(curve)
        constants = list(constants)
        h = ctx.hash_params_create(c, KIND_MIMC, len(constants), fr_to_mont(constants, c))
        return cls(ctx, c, KIND_MIMC, len(constants), h)

    @classmethod
    def poseidon(cls, ctx, curve, ark, mds, full_round, alpha: int = 5) -> "HashParams":
        """ark: rounds rows of 3; mds: 3 rows of 3; full_round: one flag per round"""
        c = get_curve(curve)
        ark = [list(row) for row in ark]
        if len(full_round) != len(ark) or any(len(row) != HASH_WIDTH for row in ark):
            raise ValueError("ark is rounds x 3 and full_round has one flag per round")
        h = ctx.hash_params_create(c, KIND_POSEIDON, len(ark), fr_to_mont([x for row in ark for x in row], c), alpha,
                                   _mds_words(mds, c), np.array([1 if f else 0 for f in full_round], dtype=np.uint8))
        return cls(ctx, c, KIND_POSEIDON, len(ark), h)

    @classmethod
    def rescue(cls, ctx, curve, constants, mds, alpha: int = 5, inv_alpha: int | None = None) -> "HashParams":
        """constants: 2 R + 1 rows of 3; inv_alpha None: alpha^-1 mod (r - 1)"""
        c = get_curve(curve)
        constants = [list(row) for row in constants]
        if len(constants) < 3 or len(constants) % 2 == 0 or any(len(row) != HASH_WIDTH for row in constants):
            raise ValueError("constants is (2 R + 1) x 3")
        rounds = (len(constants) - 1) // 2
        if inv_alpha is None:
            inv_alpha = rescue_inv_alpha(c, alpha)
        h = ctx.hash_params_create(c, KIND_RESCUE, rounds, fr_to_mont([x for row in constants for x in row], c), alpha,
                                   _mds_words(mds, c), None, inv_alpha)
        return cls(ctx, c, KIND_RESCUE, rounds, h)

    def info(self) -> dict:
        return self.ctx.hash_params_info(self.handle)

    def free(self):
        if self.handle:
            self.ctx.hash_params_free(self.handle)
            self.handle = None


def _mds_words(mds, c) -> np.ndarray:
    rows = [list(row) for row in mds]
    if len(rows) != HASH_WIDTH or any(len(row) != HASH_WIDTH for row in rows):
        raise ValueError("mds is 3 x 3")
    return fr_to_mont([x for row in rows for x in row], c)


def _download(ctx, ptr: int, n: int) -> np.ndarray:
    out = np.zeros((n, 4), dtype=np.uint64)
    ctx.d2h(out, ptr)
    return out


def blocks(params: HashParams, xl, xr) -> np.ndarray:
    """block(xl[k], xr[k]) for lists of integers -> (n, 4) Montgomery words (host convenience over fr_hash_blocks_dev)"""
    ctx, c = params.ctx, params.curve
    xl, xr = list(xl), list(xr)
    if len(xl) != len(xr):
        raise ValueError("one xr per xl")
    d_l, d_r = ctx.to_device(fr_to_mont(xl, c)), ctx.to_device(fr_to_mont(xr, c))
    try:
        ctx.fr_hash_blocks_dev(params.handle, d_l, d_r, len(xl), d_l)
        return _download(ctx, d_l, len(xl))
    finally:
        ctx.dev_free(d_l)
        ctx.dev_free(d_r)


def hash_elements(params: HashParams, messages, want_xl: bool = False):
    """The reference's `*_hash` over messages of equal length (lists of integers) -> (n, 4) Montgomery images, and with want_xl the
    state before each message's last block as well (the gadget's xl; its xr is the last element of the message)."""
    ctx, c = params.ctx, params.curve
    messages = [list(m) for m in messages]
    n, length = len(messages), len(messages[0]) if messages else 0
    if any(len(m) != length for m in messages):
        raise ValueError("the messages of one call have one length")
    d_m = ctx.to_device(fr_to_mont([x for m in messages for x in m], c))
    d_o = ctx.dev_alloc(32 * n * (2 if want_xl else 1))
    try:
        ctx.fr_hash_chain_dev(params.handle, d_m, n, length, d_o, d_o + 32 * n if want_xl else 0)
        out = _download(ctx, d_o, n * (2 if want_xl else 1))
        return (out[:n], out[n:]) if want_xl else out
    finally:
        ctx.dev_free(d_m)
        ctx.dev_free(d_o)


def hash_bytes(params: HashParams, data: bytes) -> np.ndarray:
    """the reference's `hash(b)`: bytes_to_elements, then the chain -> (4,) Montgomery words"""
    return hash_elements(params, [bytes_to_elements(data, params.curve)])[0]


def mimc_trace(params: HashParams, xl, xr, stride: int | None = None) -> np.ndarray:
    """the mimc gadget's values per block, xl, xr, then (tmp, new_xl) per round -> (n, stride, 4) Montgomery words; the elements
    of a row past 2 rounds + 2 are zero (the buffer starts zeroed, the device leaves them alone)"""
    ctx, c = params.ctx, params.curve
    xl, xr = list(xl), list(xr)
    stride = stride or 2 * params.rounds + 2
    d_l, d_r = ctx.to_device(fr_to_mont(xl, c)), ctx.to_device(fr_to_mont(xr, c))
    d_o = ctx.to_device(np.zeros((len(xl) * stride, 4), dtype=np.uint64))
    try:
        ctx.fr_mimc_trace_dev(params.handle, d_l, d_r, len(xl), d_o, stride)
        return _download(ctx, d_o, len(xl) * stride).reshape(len(xl), stride, 4)
    finally:
        for p in (d_l, d_r, d_o):
            ctx.dev_free(p)


def mimc_chain_witness_dev(ctx, params: HashParams, pre_dev: int, S: int) -> int:
    """The assignment z of circuits.mimc_chain_instance(curve, S) written on the device: the element 1, then for each of the S
    samples xl, xr and (tmp, new_xl) per round.  pre_dev: the 2 S pre-images as DEVICE Montgomery Fr, all xl first, then all xr.
    Returns the device pointer of the 1 + 12 S elements (the caller frees it): what ProvingKey.prove_raw takes with z_on_device."""
    if params.kind != KIND_MIMC or params.rounds != MIMC_ROUNDS:
        raise ValueError(f"the chain is MiMC with {MIMC_ROUNDS} rounds")
    row = 2 * MIMC_ROUNDS + 2
    z_dev = ctx.dev_alloc(32 * (1 + row * S))
    try:
        ctx.h2d(z_dev, fr_mont(1, params.curve))
        ctx.fr_mimc_trace_dev(params.handle, pre_dev, pre_dev + 32 * S, S, z_dev + 32, row)
    except Exception:
        ctx.dev_free(z_dev)
        raise
    return z_dev
