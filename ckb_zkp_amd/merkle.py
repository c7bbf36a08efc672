"""The complete binary Merkle tree of gadgets/src/merkletree/cbmt.rs on the device: build_merkle_tree (:182-202) over
zkp_fr_merkle_tree_dev and build_proof (:31-72) over zkp_fr_merkle_paths_dev, with one of hashes.HashParams as the merge.

A tree of n leaves is 2 n - 1 nodes in heap order, node i above 2 i + 1 and 2 i + 2, the leaves last; nodes[0] is the root.
MERGE_BLOCK merges with one block, block(l, r); MERGE_CHAIN with the reference's hash(l || r) = block(block(0, l), r), its MergeMimc
(cbmt_constraints.rs:146-155).  There is no CPU fallback."""
from __future__ import annotations

import numpy as np

from .codec import fr_to_mont
from .hashes import HASH_TAIL_DEPTHS, HashParams

MERGE_BLOCK, MERGE_CHAIN = 0, 1          # zkp_merge
BAD_LEAF = 0xFFFFFFFF                    # ZKP_MERKLE_BAD_LEAF


def depth(i: int) -> int:
    """depth of heap index i: floor(log2(i + 1))"""
    return (i + 1).bit_length() - 1


def launch_plan(n: int) -> list:
    """csrc/fr_hash.hpp merkle_plan: (lo, hi, tail) per launch"""
    if n < 2:
        return []
    inner = n - 1
    plan = [((1 << d) - 1, min((2 << d) - 1, inner), False) for d in range(depth(n - 2), HASH_TAIL_DEPTHS - 1, -1)]
    return plan + [(0, min(inner, (1 << HASH_TAIL_DEPTHS) - 1), True)]


class Tree:
    """2 n - 1 nodes (Montgomery Fr) in device memory of params.ctx"""

    def __init__(self, params: HashParams, n: int, nodes_dev: int):
        self.params, self.ctx, self.n, self.nodes_dev = params, params.ctx, n, nodes_dev

    def nodes(self) -> np.ndarray:
        out = np.zeros((2 * self.n - 1, 4), dtype=np.uint64)
        self.ctx.d2h(out, self.nodes_dev)
        return out

    def free(self):
        if self.nodes_dev:
            self.ctx.dev_free(self.nodes_dev)
            self.nodes_dev = None


def build_tree_dev(params: HashParams, leaves_dev: int, n: int, merge: int = MERGE_BLOCK) -> Tree:
    """n leaves as DEVICE Montgomery Fr -> Tree (one device copy of the leaves, then the launches of the plan)"""
    if n < 1:
        raise ValueError("a tree has at least one leaf")
    ctx = params.ctx
    nodes = ctx.dev_alloc(32 * (2 * n - 1))
    try:
        ctx.d2d(nodes + 32 * (n - 1), leaves_dev, 32 * n)
        ctx.fr_merkle_tree_dev(params.handle, merge, nodes, n)
    except Exception:
        ctx.dev_free(nodes)
        raise
    return Tree(params, n, nodes)


def build_tree(params: HashParams, leaves, merge: int = MERGE_BLOCK) -> Tree:
    """leaves: integers"""
    leaves = list(leaves)
    ctx = params.ctx
    d = ctx.to_device(fr_to_mont(leaves, params.curve)) if leaves else 0
    try:
        return build_tree_dev(params, d, len(leaves), merge)
    finally:
        if d:
            ctx.dev_free(d)


def root(tree: Tree) -> np.ndarray:
    out = np.zeros(4, dtype=np.uint64)
    tree.ctx.d2h(out, tree.nodes_dev)
    return out


def build_proofs(tree: Tree, leaf_indices) -> list:
    """build_proof for every index of the list, in one launch -> per index the (len, 4) Montgomery siblings from the leaf upwards"""
    idx = np.ascontiguousarray(leaf_indices, dtype=np.uint32)
    q, ctx = len(idx), tree.ctx
    if q == 0:
        return []
    stride = depth(2 * tree.n - 2)
    rows = np.zeros((q * max(stride, 1), 4), dtype=np.uint64)
    lens = np.zeros(q, dtype=np.uint32)
    d_i, d_o, d_l = ctx.to_device(idx), ctx.to_device(rows), ctx.to_device(lens)
    try:
        ctx.fr_merkle_paths_dev(tree.nodes_dev, tree.n, d_i, q, d_o, stride, d_l)
        ctx.d2h(rows, d_o)
        ctx.d2h(lens, d_l)
    finally:
        for p in (d_i, d_o, d_l):
            ctx.dev_free(p)
    if (lens == BAD_LEAF).any():
        raise IndexError(f"leaf index {int(idx[int(np.argmax(lens == BAD_LEAF))])} is outside the {tree.n} leaves")
    rows = rows.reshape(q, max(stride, 1), 4)
    return [rows[k, :int(lens[k])].copy() for k in range(q)]
