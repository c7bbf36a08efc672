"""zkp_sha256_dev / zkp_sha256_trace_dev / zkp_sha256_merkle_tree_dev on the device, bit for bit against hashlib and the Python
trace and tree of tests/sha256_ref.py.  Every buffer is framed by sentinels and compared whole, inputs included.

Lengths: the padding's edges (55 / 56: the last length of one block and the first of two; 119 / 120 likewise for three), lengths
that are no multiple of 4 (bytes instead of words), the empty message.  Counts: one lane, a wavefront less one, exactly one, one
more, and several workgroups."""
import hashlib
import random

import numpy as np
import pytest

from ckb_zkp_amd import _lib, merkle
from ckb_zkp_amd import sha256 as S
from tests import sha256_ref as ref

pytestmark = pytest.mark.gpu
SENT = 0xA5
FRAME = 16                                         # bytes of sentinel on either side; keeps the framed region 16-byte aligned
LENGTHS = [0, 1, 3, 55, 56, 63, 64, 65, 119, 120, 128]
COUNTS = [1, 63, 64, 65, 257]


def messages(n, length):
    rng = random.Random(1000 * n + length)
    return [bytes(rng.getrandbits(8) for _ in range(length)) for _ in range(n)]


def framed(payload: bytes, size: int) -> np.ndarray:
    """sentinels, `size` bytes (the payload, or sentinels where the device is to write), sentinels"""
    host = np.full(2 * FRAME + size, SENT, dtype=np.uint8)
    if payload is not None:
        host[FRAME:FRAME + size] = np.frombuffer(payload, dtype=np.uint8)
    return host


def read(ctx, ptr, like):
    got = np.zeros_like(like)
    ctx.d2h(got, ptr)
    return got


def bad_arg(fn, *args):
    with pytest.raises(_lib.ZkpError) as e:
        fn(*args)
    assert e.value.status == -1, args


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("length", LENGTHS)
def test_digests(ctx, length, n):
    msgs = messages(n, length)
    h_in, h_out = framed(b"".join(msgs), n * length), framed(None, 32 * n)
    d_in, d_out = ctx.to_device(h_in), ctx.to_device(h_out)
    try:
        ctx.sha256_dev(d_in + FRAME, n, length, d_out + FRAME)
        ctx.sync()
        want = h_out.copy()
        want[FRAME:FRAME + 32 * n] = np.frombuffer(b"".join(hashlib.sha256(m).digest() for m in msgs), dtype=np.uint8)
        assert np.array_equal(read(ctx, d_out, h_out), want)
        assert np.array_equal(read(ctx, d_in, h_in), h_in)                                  # the inputs are unchanged
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)


def test_digests_driver(ctx):
    msgs = messages(5, 33)
    assert S.digests(ctx, msgs) == [hashlib.sha256(m).digest() for m in msgs]
    assert S.digests(ctx, [b""]) == [hashlib.sha256(b"").digest()]


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("length", [0, 55, 56, 64])
def test_trace(ctx, length, n):
    msgs = messages(n, length)
    W = S.trace_words(length)
    want_t = ref.trace(msgs)
    assert want_t.shape == (W, n) and not want_t[0].any()
    h_in, h_out = framed(b"".join(msgs), n * length), framed(None, 4 * W * n)
    d_in, d_out = ctx.to_device(h_in), ctx.to_device(h_out)
    try:
        ctx.sha256_trace_dev(d_in + FRAME, n, length, d_out + FRAME)
        ctx.sync()
        want = h_out.copy()
        want[FRAME:FRAME + 4 * W * n] = want_t.reshape(-1).view(np.uint8)
        got = read(ctx, d_out, h_out)
        assert not got[FRAME:FRAME + 4 * n].any()                                           # row 0 is zero
        assert np.array_equal(got, want)
        assert np.array_equal(read(ctx, d_in, h_in), h_in)
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
    if n == 1:
        assert np.array_equal(S.trace(ctx, msgs), want_t)                                   # the driver


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 257])
def test_tree_and_paths(ctx, n):
    leaves = messages(n, 32)
    nodes = ref.cbmt(leaves)
    host = framed(None, 32 * (2 * n - 1))
    host[FRAME + 32 * (n - 1):FRAME + 32 * (2 * n - 1)] = np.frombuffer(b"".join(leaves), dtype=np.uint8)
    d = ctx.to_device(host)
    try:
        ctx.sha256_merkle_tree_dev(d + FRAME, n)
        ctx.sync()
        want = host.copy()
        want[FRAME:FRAME + 32 * (2 * n - 1)] = np.frombuffer(b"".join(nodes), dtype=np.uint8)
        assert np.array_equal(read(ctx, d, host), want)
    finally:
        ctx.dev_free(d)
    # the driver, and a path for every leaf through zkp_fr_merkle_paths_dev
    tree = merkle.build_tree_sha256(ctx, leaves)
    try:
        assert merkle.root(tree).tobytes() == nodes[0]
        assert [bytes(x) for x in tree.nodes()] == nodes
        proofs = merkle.build_proofs(tree, list(range(n)))
    finally:
        tree.free()
    for k, lemmas in enumerate(proofs):
        assert lemmas == ref.cbmt_proof(nodes, k)
        assert ref.cbmt_root(n - 1 + k, leaves[k], lemmas) == nodes[0]
        msgs = merkle.membership_messages(n - 1 + k, leaves[k], lemmas)
        assert not msgs or hashlib.sha256(msgs[-1]).digest() == nodes[0]


def test_argument_rules(ctx):
    buf = ctx.to_device(np.zeros(1 << 16, dtype=np.uint8))
    out = ctx.to_device(np.full(1 << 16, SENT, dtype=np.uint8))
    try:
        for fn in (ctx.sha256_dev, ctx.sha256_trace_dev):
            bad_arg(fn, 0, 1, 64, out)                                                      # NULL
            bad_arg(fn, buf, 1, 64, 0)
            bad_arg(fn, buf + 4, 1, 64, out)                                                # misaligned
            bad_arg(fn, buf, 1, 64, out + 8)
            bad_arg(fn, buf, 0, 64, out)                                                    # no message
            bad_arg(fn, buf, 1, (1 << S.MAX_LOG_LEN) + 1, out)                              # a message above the cap
            bad_arg(fn, buf, (1 << S.MAX_LOG_BYTES) // 65 + 1, 64, out)                     # n (len + 1) above the cap
            bad_arg(fn, buf, 2, 64, buf + 64)                                               # the output inside the messages
            bad_arg(fn, buf, 2, 64, buf + 128 - 16)
            fn(buf, 2, 64, buf + 128)                                                       # adjacent: fine
        bad_arg(ctx.sha256_trace_dev, buf, (1 << S.MAX_LOG_TRACE_WORDS) // S.trace_words(64) + 1, 64, out)
        bad_arg(ctx.sha256_merkle_tree_dev, 0, 2)
        bad_arg(ctx.sha256_merkle_tree_dev, out + 8, 2)
        bad_arg(ctx.sha256_merkle_tree_dev, out, 0)
        bad_arg(ctx.sha256_merkle_tree_dev, out, (1 << S.MAX_LOG_LEAVES) + 1)
        ctx.sync()
        got = np.zeros(1 << 16, dtype=np.uint8)
        ctx.d2h(got, out)
        assert (got == SENT).all()                                                          # nothing ran on an error
    finally:
        ctx.dev_free(buf)
        ctx.dev_free(out)
