"""SPARK memory checking on the device: `memory_in_the_head`, `memory_checking` (spartan/src/spark.rs:132-176, 209-296) and
`product_circuit_eval_prover` (prover.rs:1313-1440) with every hash, circuit layer and sum-check table resident on the device.

One zkp_fr_memcheck_circuits_dev call hashes the 2k read / write lists of n operations and builds their product circuits; a
second one does the same for init and audit over the m memory cells.  A circuit of n leaves is ONE device buffer of 2n - 2 Fr:
layer l (n >> l elements) starts at element 2n - (2n >> l), its first / second half are the reference's left_vec[l] / right_vec[l].
`product_circuit_eval_prover` walks the layers from the top and runs sumcheck.prove_cubic_batched over those halves IN PLACE: no
copies are made and the circuits are consumed.

As in sumcheck.py the commitments and the merlin transcript are the caller's; three callbacks stand where the reference draws
challenges (canonical Python integers in and out):
    next_coeffs(count)                      -> `count` integers            ("rand_coeffs_next_layer")
    next_round(coeffs)                      -> the sum-check challenge     ("challenge_nextround")
    next_layer(left, right, dotp or None)   -> r_layer                     ("challenge_r_layer"), after the caller absorbed the claims
"""
from __future__ import annotations

import numpy as np

from .api import VEC_MUL
from .codec import fr_int, fr_mont
from .params import get_curve
from .sumcheck import prove_cubic_batched


def layer_offset(n: int, l: int) -> int:
    """element at which layer l of a circuit of n leaves starts"""
    return 2 * n - ((2 * n) >> l)


def memory_in_the_head(addrs_list, m: int):
    """spark.rs:132-176: the read timestamps of every list and the audit timestamps of the m cells, as numpy uint32.
    Per-key set-up on the host.  Timestamps carry over from list to list, so they reach k n: that must stay below 2^32."""
    audit = np.zeros(m, dtype=np.int64)
    total = sum(len(a) for a in addrs_list)
    assert total < 1 << 32, "timestamps reach k * n: it must be below 2^32"
    read_ts_list = []
    for addrs in addrs_list:
        a = np.asarray(addrs, dtype=np.int64)
        assert a.ndim == 1 and (len(a) == 0 or (a.min() >= 0 and a.max() < m))
        order = np.argsort(a, kind="stable")
        s = a[order]
        first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]]) if len(s) else np.zeros(0, dtype=np.int64)
        rank = np.arange(len(s)) - np.repeat(first, np.diff(np.r_[first, len(s)]))      # earlier reads of the same cell in this list
        read = np.empty(len(a), dtype=np.int64)
        read[order] = audit[s] + rank
        audit += np.bincount(a, minlength=m)
        read_ts_list.append(read.astype(np.uint32))
    return read_ts_list, audit.astype(np.uint32)


class MemoryLayer:
    """The product circuits of one memory_checking call (DEVICE buffers) and their roots (integers)."""

    def __init__(self, n, m, init, read, write, audit, roots):
        self.n, self.m, self.init, self.read, self.write, self.audit = n, m, init, read, write, audit
        self.roots = roots                         # dict(init=, read=[...], write=[...], audit=)

    def ops(self):
        """the 2k circuits of n leaves in the order read_0, write_0, read_1, ..."""
        return [p for pair in zip(self.read, self.write) for p in pair]

    def mem(self):
        return [self.init, self.audit]

    def free(self, ctx):
        for p in self.ops() + self.mem():
            ctx.dev_free(p)
        self.read, self.write, self.init, self.audit = [], [], None, None


def memory_checking(ctx, curve, addrs_dev, mem_dev, read_ts_dev, audit_ts_dev, e_dev, n: int, m: int, gamma) -> MemoryLayer:
    """spark.rs:209-296.  addrs_dev / read_ts_dev: k DEVICE pointers to n uint32 each; e_dev: k DEVICE pointers to n Montgomery Fr
    (e_k[i] = mem[addrs_k[i]], e.g. by Context.fr_gather); mem_dev: m Montgomery Fr; audit_ts_dev: m uint32; gamma = (gamma1,
    gamma2) integers.  Two calls: the 2k circuits of n leaves, then init and audit of m leaves.
    Raises ValueError if init * prod(write) != prod(read) * audit (spark.rs:285).  The caller frees the returned MemoryLayer."""
    c = get_curve(curve)
    r = c.r
    k = len(addrs_dev)
    assert k >= 1 and len(read_ts_dev) == k and len(e_dev) == k
    g1, g2 = fr_mont(gamma[0], c), fr_mont(gamma[1], c)
    bufs = []
    try:
        for _ in range(2 * k):
            bufs.append(ctx.dev_alloc(32 * (2 * n - 2)))
        for _ in range(2):
            bufs.append(ctx.dev_alloc(32 * (2 * m - 2)))
        ops, (init, audit) = bufs[:2 * k], bufs[2 * k:]
        rep = lambda ps: [p for p in ps for _ in range(2)]                               # noqa: E731
        ops_roots = ctx.fr_memcheck_circuits_dev(c, rep(addrs_dev), rep(e_dev), rep(read_ts_dev), [0, 1] * k, ops, n, g1, g2)
        mem_roots = ctx.fr_memcheck_circuits_dev(c, [None, None], [mem_dev, mem_dev], [None, audit_ts_dev], [0, 0], [init, audit], m,
                                                 g1, g2)
        roots = dict(init=fr_int(mem_roots[0], c), audit=fr_int(mem_roots[1], c), read=[fr_int(x, c) for x in ops_roots[0::2]],
                     write=[fr_int(x, c) for x in ops_roots[1::2]])
        lhs, rhs = roots["init"], roots["audit"]
        for w, rd in zip(roots["write"], roots["read"]):
            lhs, rhs = lhs * w % r, rhs * rd % r
        if lhs != rhs:
            raise ValueError("memory check failed: init * prod(write) != prod(read) * audit")
        return MemoryLayer(n, m, init, ops[0::2], ops[1::2], audit, roots)
    except BaseException:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
        raise


def product_circuit_eval_prover(ctx, curve, circuits, n: int, dotp, next_coeffs, next_round, next_layer):
    """prover.rs:1313-1440 over DEVICE circuits of n leaves each (the buffers zkp_fr_memcheck_circuits_dev /
    zkp_fr_product_circuit_dev filled).  dotp: (row, col, val) DEVICE pointers to n / 2 Montgomery Fr each: the dot-product
    circuits that join the sum-check of layer 0 (an even number of them: the two halves of each vector).
    The circuits and the dotp vectors are bound in place: they are consumed.
    Returns (layers, claim_dotp, rands): layers = [(polys, claim_prod_left, claim_prod_right)] from the top layer down,
    claim_dotp = (rows, cols, vals) final values ([] each without dotp), rands the point the leaves are left to be opened at."""
    c = get_curve(curve)
    r = c.r
    assert circuits and n >= 2 and n & (n - 1) == 0
    layer_num = n.bit_length() - 1
    bufs = []
    try:
        # evaluate_product_circuit: the two elements of the last layer
        claims = []
        top = np.zeros((2, 4), dtype=np.uint64)
        for p in circuits:
            ctx.d2h(top, p + 32 * layer_offset(n, layer_num - 1))
            claims.append(fr_int(top[0], c) * fr_int(top[1], c) % r)
        d_eq = ctx.dev_alloc(32 * (n // 2))
        bufs.append(d_eq)
        layers, rands = [], []
        final_dotp = ([], [], [])
        for i in reversed(range(layer_num)):
            left_len = n >> (i + 1)
            lefts = [p + 32 * layer_offset(n, i) for p in circuits]
            par = [(lp, lp + 32 * left_len) for lp in lefts]
            ctx.fr_eq_evals_dev(c, np.stack([fr_mont(x, c) for x in rands]) if rands else np.zeros((0, 4), np.uint64), d_eq)
            with_dotp = i == 0 and len(dotp) > 0
            seq = []
            if with_dotp:
                seq = [tuple(t) for t in dotp]
                d_tmp = ctx.dev_alloc(32 * left_len * len(seq))
                bufs.append(d_tmp)
                tmps = [d_tmp + 32 * left_len * j for j in range(len(seq))]
                for (row, col, _), t in zip(seq, tmps):
                    ctx.fr_vec_op(c, VEC_MUL, row, col, t, left_len)
                sums = ctx.fr_dot_batch_dev(c, tmps, [val for _, _, val in seq], [left_len] * len(seq))
                claims = claims + [fr_int(s, c) for s in sums]
            coeffs = [x % r for x in next_coeffs(len(claims))]
            claim = sum(x * w for x, w in zip(claims, coeffs)) % r
            polys, rand_prod, claim_prod, claim_dotp = prove_cubic_batched(ctx, c, par, d_eq, seq, coeffs, left_len, claim, next_round)
            left, right, _ = claim_prod
            if with_dotp:
                final_dotp = claim_dotp
            r_layer = next_layer(list(left), list(right), tuple(list(t) for t in claim_dotp) if with_dotp else None) % r
            claims = [(x + r_layer * (y - x)) % r for x, y in zip(left, right)]
            rands = [r_layer] + list(rand_prod)
            layers.append((polys, list(left), list(right)))
        return layers, tuple(list(t) for t in final_dotp), rands
    finally:
        ctx.sync()
        for p in bufs:
            ctx.dev_free(p)
