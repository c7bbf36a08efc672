"""References for the SHA-256 tests, over Python integers and hashlib alone: the canonical trace that ckb_zkp_amd/sha256.py
describes, the complete binary Merkle tree with SHA-256(l || r) as the merge, and the satisfaction of an R1CS given as three CSR
matrices.  The trace is written from FIPS 180-4 and the layout, not from the gadget: the sums are kept as full integers."""
import hashlib

import numpy as np

from ckb_zkp_amd import sha256 as S
from ckb_zkp_amd.codec import fr_from_mont

M32 = 0xFFFFFFFF


def rotr(x, n):
    return (x >> n | x << (32 - n)) & M32


def pad(msg: bytes) -> bytes:
    out = msg + b"\x80"
    out += b"\x00" * (-(len(out) + 8) % 64)
    return out + (8 * len(msg)).to_bytes(8, "big")


def trace_one(msg: bytes) -> list:
    """the W words of one message's trace"""
    padded = pad(msg)
    nblocks = len(padded) // 64
    assert nblocks == S.blocks(len(msg))
    T = [0] * S.trace_words(len(msg))
    st = list(S.IV)
    for blk in range(nblocks):
        base = 1 + S.BLOCK_WORDS * blk

        def put(x, v):
            assert T[base + x] == 0 and 0 <= v <= M32
            T[base + x] = v

        def put64(x, v):
            put(x, v & M32)
            put(x + 1, v >> 32)

        w = [int.from_bytes(padded[64 * blk + 4 * j:64 * blk + 4 * j + 4], "big") for j in range(16)]
        for j in range(16):
            put(S.OFF_INPUT + j, w[j])
        for i in range(16, 64):
            x = S.OFF_SCHED + S.SCHED_WORDS * (i - 16)
            t0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18)
            s0 = t0 ^ (w[i - 15] >> 3)
            t1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19)
            s1 = t1 ^ (w[i - 2] >> 10)
            total = w[i - 16] + s0 + w[i - 7] + s1
            put(x, t0), put(x + 1, s0), put(x + 2, t1), put(x + 3, s1), put64(x + 4, total)
            w.append(total & M32)
        a, b, c, d, e, f, g, h = st
        a_sum, e_sum = a, e
        for i in range(64):
            x = S.OFF_ROUND + S.ROUND_WORDS * i
            e1 = rotr(e, 6) ^ rotr(e, 11)
            s1 = e1 ^ rotr(e, 25)
            ch = (e & f) ^ (~e & M32 & g)
            a1 = rotr(a, 2) ^ rotr(a, 13)
            s0 = a1 ^ rotr(a, 22)
            maj = (a & b) ^ (a & c) ^ (b & c)
            put64(x, e_sum), put(x + 2, e1), put(x + 3, s1), put(x + 4, ch)
            put64(x + 5, a_sum), put(x + 7, a1), put(x + 8, s0), put(x + 9, maj), put(x + 10, b & c)
            temp1 = h + s1 + ch + S.ROUND_CONSTANTS[i] + w[i]
            e_sum, a_sum = temp1 + d, temp1 + s0 + maj
            h, g, f, e = g, f, e, e_sum & M32
            d, c, b, a = c, b, a, a_sum & M32
        fin = [a_sum + st[0], st[1] + b, st[2] + c, st[3] + d, e_sum + st[4], st[5] + f, st[6] + g, st[7] + h]
        for k in range(8):
            put64(S.OFF_FINAL + 2 * k, fin[k])
        st = [v & M32 for v in fin]
    assert b"".join(v.to_bytes(4, "big") for v in st) == hashlib.sha256(msg).digest()
    return T


def trace(msgs) -> np.ndarray:
    """(W, n) uint32: T[w, k] is word w of message k"""
    return np.array([trace_one(bytes(m)) for m in msgs], dtype=np.uint32).T.copy()


def cbmt(leaves) -> list:
    """the 2 n - 1 nodes in heap order"""
    n = len(leaves)
    nodes = [b""] * (n - 1) + [bytes(x) for x in leaves]
    for i in range(n - 2, -1, -1):
        nodes[i] = hashlib.sha256(nodes[2 * i + 1] + nodes[2 * i + 2]).digest()
    return nodes


def cbmt_proof(nodes, leaf_index: int) -> list:
    i = (len(nodes) + 1) // 2 - 1 + leaf_index
    out = []
    while i > 0:
        out.append(nodes[((i + 1) ^ 1) - 1])
        i = (i - 1) >> 1
    return out


def cbmt_root(heap_index: int, leaf: bytes, lemmas) -> bytes:
    cur = leaf
    for s in lemmas:
        cur = hashlib.sha256(cur + s if heap_index & 1 else s + cur).digest()
        heap_index = (heap_index - 1) >> 1
    return cur


def is_satisfied(cs, z=None) -> bool:
    """<a_i, z> <b_i, z> == <c_i, z> (mod r) for every row of the three CSR matrices of cs"""
    r = cs.curve.r
    z = list(cs.full_assignment() if z is None else z)
    prod = []
    for which in "abc":
        row_ptr, col, coeff = cs.csr(which)
        coeff = fr_from_mont(coeff, cs.curve)
        terms = [int(c) * z[int(j)] for c, j in zip(coeff, col)]
        prod.append([sum(terms[row_ptr[i]:row_ptr[i + 1]]) % r for i in range(len(row_ptr) - 1)])
    return all(a * b % r == c for a, b, c in zip(*prod))


class MessageCircuit:
    """sha256 of one allocated message of len(data) bytes (data None: `length` bytes without values): the shape behind the
    reference's test_against_vectors, with the digest Booleans kept in .output"""
    messages = 1

    def __init__(self, data=None, length=None):
        self.data, self.message_len = data, len(data) if data is not None else length

    def generate_constraints(self, cs):
        from ckb_zkp_amd.bits import AllocatedBit, Boolean
        tags = S.input_bit_tags(0, 0, self.message_len)
        values = [None] * (8 * self.message_len) if self.data is None else S.bytes_to_bits(self.data)
        self.output = S.sha256(cs, [Boolean.is_(AllocatedBit.alloc(cs, v, tags[i])) for i, v in enumerate(values)], 0)


def bits_to_bytes(bits) -> bytes:
    return bytes(sum(int(bits[8 * k + i]) << (7 - i) for i in range(8)) for k in range(len(bits) // 8))
