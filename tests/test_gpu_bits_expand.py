"""zkp_fr_bits_expand_dev on the device against a hand-made trace and hand-made codes, bit for bit, on both curves: both
constants, complemented codes, bit 31 of a word, the last word of the last message, more codes than one workgroup has lanes, one
and three instances, and a z_stride above m whose gap stays untouched.  The buffers are framed by sentinels and compared whole."""
import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec
from ckb_zkp_amd import sha256 as S
from ckb_zkp_amd.bits import CODE_ONE, CODE_ZERO, code
from ckb_zkp_amd.params import get_curve

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xDEADBEEFCAFEF00D
W, MPI = 5, 2                                      # words per message, messages per instance: nothing here is SHA-256
GAP = 3


def hand_made(q):
    """(trace (W, q MPI) with row 0 zero, codes): the named cases first, then enough random codes for a second workgroup"""
    rng = np.random.default_rng(7 + q)
    trace = rng.integers(0, 1 << 32, size=(W, q * MPI), dtype=np.uint64).astype(np.uint32)
    trace[0] = 0
    last = W * MPI - 1
    codes = [CODE_ZERO, CODE_ONE, code(1, 0), code(1, 0, 1), code(2, 31), code(2, 31, 1), code(W + 3, 17), code(last, 31),
             code(last, 0, 1), code(W, 5, 1)]                                              # v = W: word 0 of message 1, complemented
    codes += [code(int(rng.integers(0, W * MPI)), int(rng.integers(0, 32)), int(rng.integers(0, 2)))
              for _ in range(S.EXPAND_THREADS + 37)]
    return trace, np.array(codes, dtype=np.uint32)


def expected_bits(trace, codes, q):
    out = np.zeros((q, len(codes)), dtype=np.uint8)
    for b in range(q):
        for j, c in enumerate(codes):
            v, bit, neg = int(c) >> 6, (int(c) >> 1) & 31, int(c) & 1
            out[b, j] = ((int(trace[v % W, b * MPI + v // W]) >> bit) & 1) ^ neg
    return out


def test_the_two_montgomery_ones_differ():
    assert not np.array_equal(codec.fr_mont(1, get_curve("bn254")), codec.fr_mont(1, get_curve("bls12_381")))


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("curve", CURVES)
def test_expand(ctx, curve, q):
    c = get_curve(curve)
    trace, codes = hand_made(q)
    m, stride = len(codes), len(codes) + GAP
    bits = expected_bits(trace, codes, q)
    assert bits[:, 0].sum() == 0 and bits[:, 1].all() and bits.any(axis=0).sum() > 1
    one = codec.fr_mont(1, c)
    host = np.full((1 + q * stride + 1, 4), SENT, dtype=np.uint64)
    want = host.copy()
    for b in range(q):
        want[1 + b * stride:1 + b * stride + m] = np.where(bits[b][:, None] == 1, one[None, :], np.zeros(4, dtype=np.uint64)[None, :])
    d_t, d_c, d_z = ctx.to_device(trace), ctx.to_device(codes), ctx.to_device(host)
    try:
        ctx.fr_bits_expand_dev(c, d_t, W, MPI, q, d_c, m, W * MPI - 1, d_z + 32, stride)
        ctx.sync()
        got = np.zeros_like(host)
        ctx.d2h(got, d_z)
        assert np.array_equal(got, want)                                                   # the gaps and the frame included
    finally:
        for p in (d_t, d_c, d_z):
            ctx.dev_free(p)


def test_a_code_outside_the_instance_reads_nothing(ctx):
    """max_v is the caller's word; a code past the instance's words gives its bare neg and reads nothing"""
    c = get_curve("bn254")
    trace = np.full((W, MPI), 0xFFFFFFFF, dtype=np.uint32)
    trace[0] = 0
    codes = np.array([code(W * MPI, 3), code(W * MPI + 100, 3, 1), code(1, 3)], dtype=np.uint32)
    d_t, d_c, d_z = ctx.to_device(trace), ctx.to_device(codes), ctx.to_device(np.full((3, 4), SENT, dtype=np.uint64))
    try:
        ctx.fr_bits_expand_dev(c, d_t, W, MPI, 1, d_c, 3, 1, d_z, 3)
        ctx.sync()
        got = np.zeros((3, 4), dtype=np.uint64)
        ctx.d2h(got, d_z)
        one = codec.fr_mont(1, c)
        assert not got[0].any() and np.array_equal(got[1], one) and np.array_equal(got[2], one)
    finally:
        for p in (d_t, d_c, d_z):
            ctx.dev_free(p)


def test_argument_rules(ctx):
    c = get_curve("bn254")
    trace, codes = hand_made(1)
    m = len(codes)
    host = np.full((m + 8, 4), SENT, dtype=np.uint64)
    d_t, d_c, d_z = ctx.to_device(trace), ctx.to_device(codes), ctx.to_device(host)

    def status(*args, curve=c.cid):
        return ctx.lib.zkp_fr_bits_expand_dev(ctx.h, curve, *args)

    try:
        ok = (d_t, W, MPI, 1, d_c, m, W * MPI - 1, d_z, m)
        rules = {"NULL trace": (0,) + ok[1:], "NULL codes": ok[:4] + (0,) + ok[5:], "NULL z": ok[:7] + (0, m),
                 "misaligned trace": (d_t + 4,) + ok[1:], "misaligned codes": ok[:4] + (d_c + 4,) + ok[5:],
                 "misaligned z": ok[:7] + (d_z + 8, m), "no words": (d_t, 0) + ok[2:], "no messages": (d_t, W, 0) + ok[3:],
                 "no instance": ok[:3] + (0,) + ok[4:], "no codes": ok[:5] + (0,) + ok[6:], "stride below m": ok[:8] + (m - 1,),
                 "max_v out of range": ok[:6] + (W * MPI,) + ok[7:], "words above the code cap": (d_t, (1 << S.MAX_LOG_CODE_WORDS) + 1, 1) + ok[3:],
                 "q stride above 2^32": ok[:8] + ((1 << 32) + 1,), "z over the codes": ok[:7] + (d_c, m), "z over the trace": ok[:7] + (d_t, m)}
        for name, args in rules.items():
            assert status(*args) == -1, name
        assert status(*ok, curve=7) == -2                                                  # ZKP_ERR_UNSUPPORTED_CURVE
        ctx.sync()
        got = np.zeros_like(host)
        ctx.d2h(got, d_z)
        assert (got == SENT).all()                                                         # nothing ran on an error
        assert status(*ok) == 0
        with pytest.raises(_lib.ZkpError):
            ctx.fr_bits_expand_dev(c, d_t, W, MPI, 1, d_c, m, W * MPI, d_z, m)
        ctx.sync()
    finally:
        for p in (d_t, d_c, d_z):
            ctx.dev_free(p)
