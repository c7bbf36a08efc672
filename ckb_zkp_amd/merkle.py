"""The complete binary Merkle tree of gadgets/src/merkletree/cbmt.rs on the device: build_merkle_tree (:182-202) over
zkp_fr_merkle_tree_dev and build_proof (:31-72) over zkp_fr_merkle_paths_dev, with one of hashes.HashParams as the merge.

A tree of n leaves is 2 n - 1 nodes in heap order, node i above 2 i + 1 and 2 i + 2, the leaves last; nodes[0] is the root.
MERGE_BLOCK merges with one block, block(l, r); MERGE_CHAIN with the reference's hash(l || r) = block(block(0, l), r), its MergeMimc
(cbmt_constraints.rs:146-155).  build_tree_sha256 builds the same tree over 32-byte items with SHA-256(l || r) as the merge
(gadgets/examples/merkle_tree_sha256.rs:16-28) over zkp_sha256_merkle_tree_dev; its nodes are digests, and build_proofs serves it
through the same gather.  MerkleProofGadget is the membership gadget of cbmt_constraints.rs:10-114 over sha256.py.  There is no CPU
fallback for the device entries."""
from __future__ import annotations

import hashlib

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
    """2 n - 1 nodes in device memory of the context: Montgomery Fr under params, or 32-byte digests (params None, SHA-256)"""

    def __init__(self, params: HashParams | None, n: int, nodes_dev: int, ctx=None):
        self.params, self.ctx, self.n, self.nodes_dev = params, ctx or params.ctx, n, nodes_dev

    def nodes(self) -> np.ndarray:
        """(2 n - 1, 4) uint64 Montgomery words, or (2 n - 1, 32) uint8 digests"""
        out = np.zeros((2 * self.n - 1, 4), dtype=np.uint64) if self.params else np.zeros((2 * self.n - 1, 32), dtype=np.uint8)
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


def build_tree_sha256(ctx, leaves) -> Tree:
    """leaves: byte strings of 32 bytes -> the Tree of digests, nodes[i] = SHA-256(nodes[2 i + 1] || nodes[2 i + 2])"""
    leaves = [bytes(x) for x in leaves]
    if not leaves or any(len(x) != 32 for x in leaves):
        raise ValueError("a SHA-256 tree has at least one leaf and items of 32 bytes")
    n = len(leaves)
    nodes = ctx.dev_alloc(32 * (2 * n - 1))
    try:
        ctx.h2d(nodes + 32 * (n - 1), np.frombuffer(b"".join(leaves), dtype=np.uint8))
        ctx.sha256_merkle_tree_dev(nodes, n)
    except Exception:
        ctx.dev_free(nodes)
        raise
    return Tree(None, n, nodes, ctx)


def root(tree: Tree) -> np.ndarray:
    out = np.zeros(4, dtype=np.uint64) if tree.params else np.zeros(32, dtype=np.uint8)
    tree.ctx.d2h(out, tree.nodes_dev)
    return out


def build_proofs(tree: Tree, leaf_indices) -> list:
    """build_proof for every index of the list, in one launch -> per index the (len, 4) Montgomery siblings from the leaf upwards;
    for a tree of digests, per index the list of 32-byte siblings"""
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
    if tree.params is None:
        return [[rows[k, j].tobytes() for j in range(int(lens[k]))] for k in range(q)]
    return [rows[k, :int(lens[k])].copy() for k in range(q)]


def membership_messages(index: int, leaf: bytes, lemmas) -> list:
    """The messages that a SHA-256 membership proof hashes, first to last: d = len(lemmas) strings of 64 bytes, message i the
    pair whose digest is the node i + 1 levels above the leaf.  index: the HEAP index of the leaf, n - 1 + its position, as
    MerkleProof.index (cbmt.rs:36-37); an odd index is a left child (:235-237).  d hashes on the host."""
    out, parent = [], bytes(leaf)
    for sibling in lemmas:
        out.append(parent + bytes(sibling) if index & 1 else bytes(sibling) + parent)
        parent = hashlib.sha256(out[-1]).digest()
        index = (index - 1) >> 1
    return out


class MerkleProofGadget:
    """cbmt_constraints.rs:10-114 with AbstractHashSha256 as H.  index: the heap index of the leaf; lemmas: one
    AbstractHashSha256Output per level.  words_per_msg: the trace words of one 64-byte message, where the variables are to be
    tagged with their place in the traces of membership_messages (message i at word i * words_per_msg)."""

    def __init__(self, index: int, lemmas):
        self.index, self.lemmas = index, list(lemmas)

    def set_membership(self, cs, root, leaf, words_per_msg: int | None = None):
        from .bits import CODE_ONE, CODE_ZERO, ONE, alloc_tagged
        from .r1cs import LinearCombination
        from .sha256 import AbstractHashSha256, input_bit_tags
        parent, index = leaf, self.index
        for i, sibling in enumerate(self.lemmas):
            pv, sv = parent.get_variables(), sibling.get_variables()
            is_left = bool(index & 1)
            base = None if words_per_msg is None else i * words_per_msg
            is_left_variable = alloc_tagged(cs, int(is_left), CODE_ONE if is_left else CODE_ZERO)
            input_value = (parent if is_left else sibling).get_variable_values()
            tags = None if base is None else input_bit_tags(base, 0, len(input_value) // 8)
            input_variables = [alloc_tagged(cs, v, None if tags is None else tags[j]) for j, v in enumerate(input_value)]
            for j in range(min(len(pv), len(sv))):
                # is_left (left - right) = input - right
                cs.enforce(lambda lc: LinearCombination([(is_left_variable, 1)]), lambda lc: LinearCombination([(pv[j], 1), (sv[j], -1)]),
                           lambda lc: LinearCombination([(input_variables[j], 1), (sv[j], -1)]))
            parent = AbstractHashSha256.hash_enforce(cs, [parent, sibling] if is_left else [sibling, parent], base)
            index = (index - 1) >> 1
        for i, j in zip(parent.get_variables(), root.get_variables()):
            cs.enforce(lambda lc: LinearCombination([(i, 1)]), lambda lc: LinearCombination([(ONE, 1)]),
                       lambda lc: LinearCombination([(j, 1)]))
