"""SHA-256 of the reference's gadgets package: the gadget over bits.py (gadgets/src/hashes/sha256.rs:34-249, :252-370), the plan
that maps a synthesised circuit's variables to bits of the canonical trace, and the drivers over zkp_sha256_dev /
zkp_sha256_trace_dev / zkp_fr_bits_expand_dev that write digests, traces and a bit circuit's witness on the device.

The canonical trace of n messages of `length` bytes is uint32 T[w * n + k], word w < trace_words(length), message k < n.  Word 0 is
0.  Block b of the padded message owns the BLOCK_WORDS words from 1 + BLOCK_WORDS * b:
    OFF_INPUT + j            j < 16: the block's input words
    OFF_SCHED + 6 (i - 16)   i = 16 .. 63: rotr7 ^ rotr18 of w[i-15]; that ^ shr3; rotr17 ^ rotr19 of w[i-2]; that ^ shr10; the sum
                             w[i-16] + s0 + w[i-7] + s1 as lo, hi
    OFF_ROUND + 11 i         i < 64: the sum that forms e as lo, hi; rotr6 ^ rotr11 of e; that ^ rotr25; ch; the sum that forms a as
                             lo, hi; rotr2 ^ rotr13 of a; that ^ rotr22; maj; b & c.  Round 0: the incoming state words, hi = 0
    OFF_FINAL + 2 k          k < 8: the sum h_k as lo, hi
The sums are the full integers: the gadget allocates their carry bits.  csrc/sha256.hpp mirrors these constants and
zkp_sha256_info reports them.  There is no CPU fallback for the drivers."""
from __future__ import annotations

import numpy as np

from .bits import CODE_WORD_BITS, AllocatedBit, Boolean, MultiEq, TaggedConstraintSystem, UInt32, code

BLOCK_WORDS = 1024                         # ZKP_SHA256_BLOCK_WORDS
OFF_INPUT, OFF_SCHED, SCHED_WORDS, OFF_ROUND, ROUND_WORDS, OFF_FINAL = 0, 16, 6, 304, 11, 1008
MAX_LOG_LEN, MAX_LOG_BYTES, MAX_LOG_TRACE_WORDS, MAX_LOG_LEAVES, MAX_LOG_CODE_WORDS = 20, 34, 32, 27, CODE_WORD_BITS
THREADS, EXPAND_THREADS = 64, 256

ROUND_CONSTANTS = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def blocks(length: int) -> int:
    return (length + 9 + 63) // 64


def trace_words(length: int) -> int:
    """W: the words of one message's trace"""
    return 1 + BLOCK_WORDS * blocks(length)


# ---- where the bytes of a message and of its digest sit in the trace
def input_bit_tags(msg_base: int, byte_offset: int, nbytes: int) -> list:
    """the codes of the bits, most significant first, of the bytes [byte_offset, byte_offset + nbytes) of the message whose trace
    starts at word msg_base"""
    out = []
    for p in range(8 * byte_offset, 8 * (byte_offset + nbytes)):
        blk, q = divmod(p, 512)
        out.append(code(msg_base + 1 + BLOCK_WORDS * blk + OFF_INPUT + q // 32, 31 - q % 32))
    return out


def digest_bit_tags(msg_base: int, length: int) -> list:
    """the codes of the 256 digest bits of the message of `length` bytes whose trace starts at word msg_base: the low words of the
    last block's final sums"""
    last = msg_base + 1 + BLOCK_WORDS * (blocks(length) - 1) + OFF_FINAL
    return [code(last + 2 * (p // 32), 31 - p % 32) for p in range(256)]


# ---- the gadget
def get_sha256_iv() -> list:
    return [UInt32.constant(v) for v in IV]


def sha256_compression_function(cs, input_bits, current_hash_value, base=None) -> list:
    """sha256.rs:82-249.  base: the trace word where this block's record starts (None: nothing is tagged)."""
    assert len(input_bits) == 512 and len(current_hash_value) == 8

    def at(off):
        return None if base is None else base + off

    w = [UInt32.from_bits_be(input_bits[32 * j:32 * j + 32]) for j in range(16)]
    with MultiEq(cs) as meq:                                       # dropped at the end of the compression (:98)
        for i in range(16, 64):
            x = OFF_SCHED + SCHED_WORDS * (i - 16)
            s0 = w[i - 15].rotr(7).xor(meq, w[i - 15].rotr(18), at(x))
            s0 = s0.xor(meq, w[i - 15].shr(3), at(x + 1))
            s1 = w[i - 2].rotr(17).xor(meq, w[i - 2].rotr(19), at(x + 2))
            s1 = s1.xor(meq, w[i - 2].shr(10), at(x + 3))
            w.append(UInt32.addmany(meq, [w[i - 16], s0, w[i - 7], s1], at(x + 4)))

        def compute(maybe, others, word):                         # Maybe::compute (:135-150): a list is deferred
            return UInt32.addmany(meq, maybe + others, word) if isinstance(maybe, list) else maybe

        a, b, c, d, e, f, g, h = current_hash_value
        for i in range(64):
            x = OFF_ROUND + ROUND_WORDS * i
            new_e = compute(e, [], at(x))
            s1 = new_e.rotr(6).xor(meq, new_e.rotr(11), at(x + 2))
            s1 = s1.xor(meq, new_e.rotr(25), at(x + 3))
            ch = UInt32.sha256_ch(meq, new_e, f, g, at(x + 4))
            temp1 = [h, s1, ch, UInt32.constant(ROUND_CONSTANTS[i]), w[i]]
            new_a = compute(a, [], at(x + 5))
            s0 = new_a.rotr(2).xor(meq, new_a.rotr(13), at(x + 7))
            s0 = s0.xor(meq, new_a.rotr(22), at(x + 8))
            maj = UInt32.sha256_maj(meq, new_a, b, c, at(x + 9), at(x + 10))
            h, g, f, e = g, f, new_e, temp1 + [d]
            d, c, b, a = c, b, new_a, temp1 + [s0, maj]
        cur = current_hash_value
        h0 = compute(a, [cur[0]], at(OFF_FINAL))
        h1 = UInt32.addmany(meq, [cur[1], b], at(OFF_FINAL + 2))
        h2 = UInt32.addmany(meq, [cur[2], c], at(OFF_FINAL + 4))
        h3 = UInt32.addmany(meq, [cur[3], d], at(OFF_FINAL + 6))
        h4 = compute(e, [cur[4]], at(OFF_FINAL + 8))
        h5 = UInt32.addmany(meq, [cur[5], f], at(OFF_FINAL + 10))
        h6 = UInt32.addmany(meq, [cur[6], g], at(OFF_FINAL + 12))
        h7 = UInt32.addmany(meq, [cur[7], h], at(OFF_FINAL + 14))
    return [h0, h1, h2, h3, h4, h5, h6, h7]


def _digest_bits(words) -> list:
    return [b for word in words for b in word.into_bits_be()]


def sha256_block_no_padding(cs, input_bits, msg_base=None) -> list:
    """sha256.rs:34-51: one compression from the IV -> 256 Booleans.  msg_base: word 0 of the trace of the 64-byte message whose
    first block this is."""
    assert len(input_bits) == 512
    return _digest_bits(sha256_compression_function(cs, input_bits, get_sha256_iv(), None if msg_base is None else msg_base + 1))


def sha256(cs, input_bits, msg_base=None) -> list:
    """sha256.rs:53-80: the padded hash of a whole number of bytes, given as bits (most significant first) -> 256 Booleans"""
    assert len(input_bits) % 8 == 0
    padded = list(input_bits)
    plen = len(padded)
    padded.append(Boolean.constant(True))
    while (len(padded) + 64) % 512 != 0:
        padded.append(Boolean.constant(False))
    padded += [Boolean.constant((plen >> i) & 1) for i in range(63, -1, -1)]
    cur = get_sha256_iv()
    for blk in range(len(padded) // 512):
        cur = sha256_compression_function(cs, padded[512 * blk:512 * blk + 512], cur,
                                          None if msg_base is None else msg_base + 1 + BLOCK_WORDS * blk)
    return _digest_bits(cur)


def bytes_to_bits(data: bytes) -> list:
    return [bool((byte >> i) & 1) for byte in data for i in range(7, -1, -1)]


class AbstractHashSha256Output:
    """sha256.rs:252-331: the bits of some bytes as variables.  data: the bytes, or their count where the values are missing."""

    def __init__(self, value, variables):
        self.value, self.variables = value, variables

    @classmethod
    def _alloc(cls, cs, data, tags, public):
        values = [None] * (8 * data) if isinstance(data, int) else bytes_to_bits(data)
        fn = AllocatedBit.alloc_input if public else AllocatedBit.alloc
        bits = [fn(cs, v, None if tags is None else tags[i]) for i, v in enumerate(values)]
        return cls([Boolean.is_(b) for b in bits], [b.variable for b in bits])

    @classmethod
    def alloc(cls, cs, data, tags=None):
        return cls._alloc(cs, data, tags, False)

    @classmethod
    def alloc_input(cls, cs, data, tags=None):
        return cls._alloc(cs, data, tags, True)

    def get_variables(self) -> list:
        return list(self.variables)

    def get_variable_values(self) -> list:
        return [None if b.get_value() is None else int(b.get_value()) for b in self.value]


class AbstractHashSha256:
    @staticmethod
    def hash_enforce(cs, params, msg_base=None) -> AbstractHashSha256Output:
        """sha256.rs:337-369: the digest of the concatenated params, and one fresh bit per digest bit (`bit_i`, :351-360)"""
        inputs = [b for o in params for b in o.value]
        booleans = sha256(cs, inputs, msg_base)
        tags = None if msg_base is None else digest_bit_tags(msg_base, len(inputs) // 8)
        variables = [AllocatedBit.alloc(cs, b.get_value(), None if tags is None else tags[i]).variable for i, b in enumerate(booleans)]
        return AbstractHashSha256Output(booleans, variables)


# ---- the plan
class WitnessPlan:
    """One code per element of z (inputs first, z[0] the constant 1) over the traces of `messages` messages of `message_len` bytes
    per instance: element j is bit `code >> 1 & 31` of word `code >> 6` of the instance's concatenated traces, complemented where
    `code & 1`."""

    def __init__(self, codes, messages: int, message_len: int):
        self.codes = np.ascontiguousarray(codes, dtype=np.uint32)
        self.messages, self.message_len = messages, message_len

    @property
    def words_per_msg(self) -> int:
        return trace_words(self.message_len)

    @property
    def max_v(self) -> int:
        return int(self.codes.max() >> 6)

    @classmethod
    def from_cs(cls, cs: TaggedConstraintSystem, messages: int, message_len: int) -> "WitnessPlan":
        tags = cs.tags()
        missing = [j for j, t in enumerate(tags) if t is None]
        if missing:
            raise ValueError(f"{len(missing)} variables carry no code, the first at z[{missing[0]}]")
        plan = cls(tags, messages, message_len)
        if plan.max_v >= plan.words_per_msg * messages:
            raise ValueError("a code points past the instance's traces")
        return plan

    def __eq__(self, other):
        return (isinstance(other, WitnessPlan) and self.messages == other.messages and self.message_len == other.message_len and
                np.array_equal(self.codes, other.codes))

    def apply(self, trace, instance: int = 0) -> list:
        """z of one instance as 0 / 1 integers from a host trace of shape (W, n): what the expand kernel computes"""
        t = np.asarray(trace, dtype=np.uint32).reshape(self.words_per_msg, -1)
        v = (self.codes >> 6).astype(np.int64)
        word = t[v % self.words_per_msg, instance * self.messages + v // self.words_per_msg]
        return [int(x) for x in ((word >> ((self.codes >> 1) & 31)) ^ self.codes) & 1]


def synthesize(circuit, curve, assign: bool = True):
    """circuit.generate_constraints over a TaggedConstraintSystem -> (cs, WitnessPlan); the circuit names its messages"""
    cs = TaggedConstraintSystem(curve, assign)
    circuit.generate_constraints(cs)
    return cs, WitnessPlan.from_cs(cs, circuit.messages, circuit.message_len)


# ---- drivers
def info() -> dict:
    """zkp_sha256_info"""
    import ctypes as C

    from . import _lib
    a = (C.c_uint64 * 16)()
    _lib.check(_lib.load().zkp_sha256_info(a), "zkp_sha256_info")
    names = ("block_words", "off_input", "off_sched", "sched_words", "off_round", "round_words", "off_final", "max_log_len",
             "max_log_bytes", "max_log_trace_words", "max_log_leaves", "max_log_code_words", "threads", "expand_threads")
    return dict(zip(names, (int(x) for x in a)))


def _upload_messages(ctx, msgs):
    msgs = [bytes(m) for m in msgs]
    if not msgs or any(len(m) != len(msgs[0]) for m in msgs):
        raise ValueError("the messages of one call are at least one and have one length")
    flat = np.frombuffer(b"".join(msgs) + bytes(16), dtype=np.uint8)                      # never an empty allocation
    return ctx.to_device(flat), len(msgs), len(msgs[0])


def digests_dev(ctx, msgs_dev: int, n: int, length: int) -> int:
    """n DEVICE messages of `length` bytes, row-major -> device pointer of the n * 32 digest bytes (the caller frees it)"""
    out = ctx.dev_alloc(32 * n)
    try:
        ctx.sha256_dev(msgs_dev, n, length, out)
    except Exception:
        ctx.dev_free(out)
        raise
    return out


def digests(ctx, msgs) -> list:
    """SHA-256 of byte strings of one length -> their digests (host convenience over digests_dev)"""
    d_m, n, length = _upload_messages(ctx, msgs)
    try:
        d_o = digests_dev(ctx, d_m, n, length)
        try:
            out = np.zeros(32 * n, dtype=np.uint8)
            ctx.d2h(out, d_o)
        finally:
            ctx.dev_free(d_o)
    finally:
        ctx.dev_free(d_m)
    return [out[32 * k:32 * k + 32].tobytes() for k in range(n)]


def trace_dev(ctx, msgs_dev: int, n: int, length: int) -> int:
    """-> device pointer of the trace_words(length) * n uint32 of the canonical trace (the caller frees it)"""
    out = ctx.dev_alloc(4 * trace_words(length) * n)
    try:
        ctx.sha256_trace_dev(msgs_dev, n, length, out)
    except Exception:
        ctx.dev_free(out)
        raise
    return out


def trace(ctx, msgs) -> np.ndarray:
    """the canonical trace of byte strings of one length as a (W, n) array (host convenience over trace_dev)"""
    d_m, n, length = _upload_messages(ctx, msgs)
    try:
        d_t = trace_dev(ctx, d_m, n, length)
        try:
            out = np.zeros((trace_words(length), n), dtype=np.uint32)
            ctx.d2h(out, d_t)
        finally:
            ctx.dev_free(d_t)
    finally:
        ctx.dev_free(d_m)
    return out


class PlanDev:
    """a WitnessPlan's codes resident on the device of `ctx`, with the largest word index among them, computed once here"""

    def __init__(self, ctx, plan: WitnessPlan):
        self.ctx, self.plan, self.m, self.max_v = ctx, plan, len(plan.codes), plan.max_v
        self.codes_dev = ctx.to_device(plan.codes)

    def free(self):
        if self.codes_dev:
            self.ctx.dev_free(self.codes_dev)
            self.codes_dev = None


def upload_plan(ctx, plan: WitnessPlan) -> PlanDev:
    return PlanDev(ctx, plan)


def witness_dev(ctx, curve, plan_dev: PlanDev, msgs_dev: int, q: int, z_stride: int | None = None) -> int:
    """The assignments z of q instances of a bit circuit written on the device: msgs_dev holds the q * plan.messages messages of
    plan.message_len bytes, those of instance b first to last at [b * messages, (b + 1) * messages).  One trace launch, one expand
    launch, one allocation for z.  Returns the device pointer of q * z_stride Montgomery Fr (z_stride defaults to the plan's
    length; the caller frees it): instance b's z at element b * z_stride, what ProvingKey.prove_raw takes with z_on_device."""
    plan = plan_dev.plan
    z_stride = z_stride or plan_dev.m
    n = q * plan.messages
    t_dev = trace_dev(ctx, msgs_dev, n, plan.message_len)
    z_dev = 0
    try:
        z_dev = ctx.dev_alloc(32 * q * z_stride)
        ctx.fr_bits_expand_dev(curve, t_dev, plan.words_per_msg, plan.messages, q, plan_dev.codes_dev, plan_dev.m, plan_dev.max_v,
                               z_dev, z_stride)
        ctx.sync()                                                 # the trace is freed below
    except Exception:
        if z_dev:
            ctx.dev_free(z_dev)
        raise
    finally:
        ctx.dev_free(t_dev)
    return z_dev

