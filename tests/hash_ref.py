"""Python-integer restatement of the reference's algebraic hashes and its complete binary Merkle tree: mimc_block / poseidon_block /
rescue_block and their `*_hash` chain (gadgets/src/hashes/{mimc,poseidon,rescue}.rs), the values the mimc gadget allocates
(mimc.rs:110-157), and CBMT (gadgets/src/merkletree/cbmt.rs): build_merkle_tree, build_proof, MerkleProof::root and the queue
algorithm build_merkle_root as a second route to the root.  The checker of ckb_zkp_amd.hashes / ckb_zkp_amd.merkle: it shares no
code with them and takes every constant as an argument.

A parameter set is a dict: {"kind": "mimc", "r", "constants"}, {"kind": "poseidon", "r", "alpha", "ark", "mds", "full"} or
{"kind": "rescue", "r", "alpha", "inv_alpha", "constants", "mds"}."""
from collections import deque

M = 3


def mimc_block(xl, xr, constants, r):
    for c in constants:
        t = (xl + c) % r
        xl, xr = (t * t % r * t + xr) % r, xl
    return xl


def mix(state, mds, r):
    return [sum(mds[j][k] * state[k] for k in range(M)) % r for j in range(M)]


def poseidon_block(xl, xr, ark, mds, full, alpha, r):
    state = [xl % r, xr % r, 0]
    for i, row in enumerate(ark):
        state = [(s + a) % r for s, a in zip(state, row)]
        if full[i]:
            state = [pow(s, alpha, r) for s in state]
        else:
            state[M - 1] = pow(state[M - 1], alpha, r)
        state = mix(state, mds, r)
    return state[0]


def poseidon_block_all_full(xl, xr, ark, mds, alpha, r):
    """the permutation with no partial round, written without a flag"""
    state = [xl % r, xr % r, 0]
    for row in ark:
        state = mix([pow((s + a) % r, alpha, r) for s, a in zip(state, row)], mds, r)
    return state[0]


def rescue_block(xl, xr, constants, mds, alpha, inv_alpha, r):
    rounds = (len(constants) - 1) // 2
    state = [(xl + constants[0][0]) % r, (xr + constants[0][1]) % r, constants[0][2] % r]
    for i in range(2 * rounds):
        e = inv_alpha if i % 2 else alpha
        state = mix([pow(s, e, r) for s in state], mds, r)
        state = [(s + c) % r for s, c in zip(state, constants[i + 1])]
    return state[0]


def block(p, xl, xr):
    if p["kind"] == "mimc":
        return mimc_block(xl, xr, p["constants"], p["r"])
    if p["kind"] == "poseidon":
        return poseidon_block(xl, xr, p["ark"], p["mds"], p["full"], p["alpha"], p["r"])
    return rescue_block(xl, xr, p["constants"], p["mds"], p["alpha"], p["inv_alpha"], p["r"])


def hash_elements(p, msg):
    """`*_hash`: -> (xl, xr, image) with xl the state before the last block and xr the last element"""
    h, xl = 0, 0
    for i, m in enumerate(msg):
        if i == len(msg) - 1:
            xl = h
        h = block(p, h, m)
    return xl, msg[-1], h


def mimc_trace(xl, xr, constants, r):
    """xl, xr, then per round tmp = (xl + c)^2 and the new xl: the allocation order of the mimc gadget"""
    out = [xl % r, xr % r]
    for c in constants:
        t = (xl + c) % r
        tmp = t * t % r
        xl, xr = (t * tmp + xr) % r, xl
        out += [tmp, xl]
    return out


def products_of_block(p, window=2):
    """Fr products of one block as csrc/fr_hash.hip schedules them (zkp_hash_params_info info[5])"""
    ap = {3: 2, 5: 3, 7: 4}
    if p["kind"] == "mimc":
        return 2 * len(p["constants"])
    if p["kind"] == "poseidon":
        return sum(ap[p["alpha"]] * (M if f else 1) + M * M for f in p["full"])
    e = p["inv_alpha"]
    digits = []
    while e:
        digits.append(e & ((1 << window) - 1))
        e >>= window
    inv = M * (((1 << window) - 2) + (len(digits) - 1) * window + sum(1 for d in digits[:-1] if d))
    return ((len(p["constants"]) - 1) // 2) * (M * ap[p["alpha"]] + inv + 2 * M * M)


# ---- CBMT
def merge_block(p):
    return lambda left, right: block(p, left, right)


def merge_chain(p):
    return lambda left, right: block(p, block(p, 0, left), right)


def build_tree(leaves, merge):
    """build_merkle_tree (cbmt.rs:182-202): 2 n - 1 nodes, the leaves last"""
    n = len(leaves)
    if n == 0:
        return []
    nodes = [0] * (n - 1) + list(leaves)
    for i in range(n - 2, -1, -1):
        nodes[i] = merge(nodes[2 * i + 1], nodes[2 * i + 2])
    return nodes


def build_merkle_root(leaves, merge):
    """the queue algorithm (cbmt.rs:158-180)"""
    if not leaves:
        return 0
    queue = deque()
    k = len(leaves)
    while k >= 2:                                       # rchunks_exact(2): pairs from the right, each in its own order
        queue.append(merge(leaves[k - 2], leaves[k - 1]))
        k -= 2
    if k == 1:
        queue.appendleft(leaves[0])
    while len(queue) > 1:
        right = queue.popleft()
        left = queue.popleft()
        queue.append(merge(left, right))
    return queue.popleft()


def sibling(i):
    return 0 if i == 0 else ((i + 1) ^ 1) - 1


def parent(i):
    return 0 if i == 0 else (i - 1) >> 1


def build_proof(nodes, leaf_index):
    """build_proof (cbmt.rs:31-72) -> (heap index, lemmas) or None"""
    if not nodes:
        return None
    n = (len(nodes) >> 1) + 1
    index = n + leaf_index - 1
    if index >= 2 * n - 1:
        return None
    lemmas = []
    if index == 0:
        return index, lemmas
    i = index
    while True:
        lemmas.append(nodes[sibling(i)])
        if parent(i) == 0:
            break
        i = parent(i)
    return index, lemmas


def proof_root(index, lemmas, leaf, merge):
    """MerkleProof::root (cbmt.rs:106-129)"""
    if index == 0 and lemmas:
        return None
    node = leaf
    for s in lemmas:
        node = merge(node, s) if index & 1 else merge(s, node)
        index = parent(index)
    return node
