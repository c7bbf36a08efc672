"""zkp_g1_scale_vec_dev / zkp_g1_ntt_dev on the device, bit-exact against Python integers (tests/g1_ntt_ref.py): the inputs are
P_j = [a_j] G with known exponents, so the expected outputs are [s_j a_j] G and [sum_j w^(i j) a_j] G.  Every writable buffer is framed
by one sentinel point / flag before and after it, whole buffers are compared word for word, and inputs of calls that are not in place
are read back unchanged.

Sizes: scale_vec at one lane, one short of a wave, a wave, one over and two waves plus one; the transform at every log_n from 1 (one
butterfly, no multiplication at all) over 7 (exactly one wave of butterflies) to 9 (four workgroups), and 12 once.  The window width
of a launch follows its grid (g1_ntt.hip pick_window): on the 256 CUs of an MI355X the 4-bit tables serve up to 256 (BLS12-381) / 512
(BN254) waves, the 3-bit ones up to 512 / 768, the 2-bit ones everything above, so scale_vec runs once just past each of these counts
and the transform once at 2^17 (2^16 butterflies: 1024 waves), against zkp_fixed_base_mul_g1 and zkp_ntt.  The structured
inputs reach the exceptional additions: equal inputs make stage 0 double and leave identities everywhere but output 0, alternating
signs make it add opposite points, identities by flag and by (0, 0) words enter as either operand."""
import ctypes as C
import random

import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec
from ckb_zkp_amd.api import NTT_FFT, NTT_IFFT
from ckb_zkp_amd.asvc import G1_NTT_MAX_LOG
from ckb_zkp_amd.params import get_curve
from tests import g1_ntt_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xDEADBEEFCAFEF00D
SENT_FLAG = 0xA5


def _bad(fn, status=-1):
    with pytest.raises(_lib.ZkpError) as e:
        fn()
    assert e.value.status == status


class Framed:
    """a device buffer of rows between two sentinel rows"""

    def __init__(self, ctx, rows: np.ndarray, sentinel):
        self.ctx = ctx
        frame = np.full((1,) + rows.shape[1:], sentinel, dtype=rows.dtype)
        self.host = np.concatenate([frame, rows, frame])
        self.dev = ctx.to_device(self.host)
        self.ptr = self.dev + self.host[0].nbytes

    def read(self):
        got = np.zeros_like(self.host)
        self.ctx.d2h(got, self.dev)
        assert np.array_equal(got[0], self.host[0]) and np.array_equal(got[-1], self.host[-1]), "a write outside the buffer"
        return got[1:-1]

    def unchanged(self):
        return np.array_equal(self.read(), self.host[1:-1])

    def free(self):
        self.ctx.dev_free(self.dev)


def framed_points(ctx, xy, inf):
    return Framed(ctx, np.ascontiguousarray(xy, dtype=np.uint64), SENT), Framed(ctx, np.ascontiguousarray(inf, dtype=np.uint8), SENT_FLAG)


def transform(ctx, c, xy, inf, op):
    """the entry over sentinel-framed copies -> (xy, inf)"""
    bx, bi = framed_points(ctx, xy, inf)
    try:
        ctx.g1_ntt_dev(c, bx.ptr, bi.ptr, len(xy).bit_length() - 1, op)
        return bx.read(), bi.read()
    finally:
        bx.free()
        bi.free()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------- scale_vec
def special_scalars(r):
    """0, 1, 2, r - 1, (r - 1) / 2, 2^k - 1 and 2^k at the boundaries of the 2-, 3- and 4-bit windows, and words whose windows all
    sit on the signed digits' edge (every 4-bit window 8: the largest positive digit; 7 / 9: either side of it; all ones: a carry
    through every window)"""
    out = [0, 1, 2, r - 1, (r - 1) // 2]
    for k in (2, 3, 4, 32, 33, 64, 126, 128, 129, 252, 253):
        out += [(1 << k) - 1, 1 << k]
    for nibble in (0x8, 0x7, 0x9, 0xF, 0x4, 0x5, 0x2, 0x3):
        out.append(int(f"{nibble:x}" * 64, 16) % r)
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("curve", CURVES)
def test_scale_vec(ctx, curve, n):
    c = get_curve(curve)
    rng = random.Random(f"g1-scale-{curve}-{n}")
    pool = special_scalars(c.r)
    scalars = [pool[(i + 3 * n) % len(pool)] if i < len(pool) else rng.randrange(c.r) for i in range(n)]
    exps = [rng.randrange(1, c.r) for _ in range(n)]
    xy, inf = ref.points(curve, exps)
    by_flag, by_words = (1, 2) if n > 2 else (None, None)
    if n > 2:
        inf[by_flag] = 1                                             # the words stay those of a real point
        xy[by_words] = 0                                             # flag 0
    want = ref.points(curve, [0 if i in (by_flag, by_words) else s * a for i, (s, a) in enumerate(zip(scalars, exps))])
    sc = Framed(ctx, codec.fr_to_mont(scalars, c).reshape(n, 4), SENT)
    bx, bi = framed_points(ctx, xy, inf)
    ox, oi = framed_points(ctx, np.full_like(xy, SENT), np.full_like(inf, SENT_FLAG))
    try:
        ctx.g1_scale_vec_dev(c, bx.ptr, bi.ptr, sc.ptr, n, ox.ptr, oi.ptr)           # out of place
        assert same((ox.read(), oi.read()), want), (curve, n, "out of place")
        assert bx.unchanged() and bi.unchanged() and sc.unchanged(), "an input changed"
        ctx.g1_scale_vec_dev(c, bx.ptr, bi.ptr, sc.ptr, n, bx.ptr, bi.ptr)           # in place
        assert same((bx.read(), bi.read()), want), (curve, n, "in place")
        assert sc.unchanged()
    finally:
        for b in (sc, bx, bi, ox, oi):
            b.free()
    if n == 65:                                                      # no flags at all: only the (0, 0) words mark an identity
        xy2 = xy.copy()
        xy2[by_flag] = 0
        assert same(ctx.g1_scale_vec(c, xy2, None, codec.fr_to_mont(scalars, c).reshape(n, 4)), want)
    assert ctx.g1_scale_vec_dev(c, 0, 0, 0, 0, 0, 0) is None        # n == 0: nothing runs


def device_points(ctx, c, curve, exps):
    """[e] G through zkp_fixed_base_mul_g1, for sizes where Python scalar multiplications would take minutes"""
    return ctx.fixed_base_mul(c, 1, ref.points(curve, [1])[0][0], codec.fr_canonical(exps, c))


@pytest.mark.parametrize("waves", [257, 513, 769])
@pytest.mark.parametrize("curve", CURVES)
def test_scale_vec_window_widths(ctx, curve, waves):
    """one lane into the first wave past a change of window width; in place"""
    c = get_curve(curve)
    n = (waves - 1) * 64 + 1
    rng = random.Random(f"g1-scale-width-{curve}-{waves}")
    pool = special_scalars(c.r)
    scalars = [pool[i] if i < len(pool) else rng.randrange(c.r) for i in range(n)]
    exps = [rng.randrange(1, c.r) for _ in range(n)]
    exps[n - 1] = 0
    xy, inf = device_points(ctx, c, curve, exps)
    want = device_points(ctx, c, curve, [s * a % c.r for s, a in zip(scalars, exps)])
    assert same(ctx.g1_scale_vec(c, xy, inf, codec.fr_to_mont(scalars, c).reshape(n, 4)), want)


# ------------------------------------------------------------------------------------------- the transform
def input_cases(c, n, rng):
    """name -> exponents a_j (0 = the identity, flagged)"""
    a = rng.randrange(1, c.r)
    single = [0] * n
    single[rng.randrange(n)] = rng.randrange(1, c.r)
    half = [rng.randrange(1, c.r) if rng.random() < 0.5 else 0 for _ in range(n)]
    return {"random": [rng.randrange(1, c.r) for _ in range(n)],
            "equal": [a] * n,                                        # outputs 1 .. n-1 are identities, stage 0 doubles
            "alternating": [a if j % 2 == 0 else c.r - a for j in range(n)],
            "single": single,
            "identities": [0] * n,
            "half_identities": half}


@pytest.mark.parametrize("log_n", range(1, 10))
@pytest.mark.parametrize("curve", CURVES)
def test_transform(ctx, curve, log_n):
    c = get_curve(curve)
    n = 1 << log_n
    rng = random.Random(f"g1-ntt-{curve}-{log_n}")
    for name, exps in input_cases(c, n, rng).items():
        xy, inf = ref.points(curve, exps)
        fwd = transform(ctx, c, xy, inf, NTT_FFT)
        assert same(fwd, ref.points(curve, ref.fr_transform(curve, exps, False))), (curve, log_n, name, "forward")
        inv = transform(ctx, c, xy, inf, NTT_IFFT)
        assert same(inv, ref.points(curve, ref.fr_transform(curve, exps, True))), (curve, log_n, name, "inverse")
        assert same(transform(ctx, c, fwd[0], fwd[1], NTT_IFFT), (xy, inf)), (curve, log_n, name, "forward then inverse")
        if name == "random":                                         # the root is the one zkp_ntt_dev uses
            on_dev = codec.fr_from_mont(ctx.ntt(c, codec.fr_to_mont(exps, c).reshape(n, 4), NTT_FFT), c)
            assert same(fwd, ref.points(curve, on_dev)), (curve, log_n, "root")


@pytest.mark.parametrize("curve", CURVES)
def test_transform_4096(ctx, curve):
    """log_n = 12 once: inputs and expected outputs through zkp_fixed_base_mul_g1 of the Python Fr transform"""
    c = get_curve(curve)
    n = 1 << 12
    rng = random.Random(f"g1-ntt-{curve}-12")
    exps = [rng.randrange(c.r) for _ in range(n)]
    exps[5] = 0
    g = ref.points(curve, [1])[0][0]
    xy, inf = ctx.fixed_base_mul(c, 1, g, codec.fr_canonical(exps, c))
    want = ctx.fixed_base_mul(c, 1, g, codec.fr_canonical(ref.fr_transform(curve, exps, False), c))
    fwd = transform(ctx, c, xy, inf, NTT_FFT)
    assert same(fwd, want)
    assert same(transform(ctx, c, fwd[0], fwd[1], NTT_IFFT), (xy, inf))


@pytest.mark.parametrize("curve", CURVES)
def test_transform_narrow_windows(ctx, curve):
    """log_n = 17 once: 1024 waves of butterflies, past the 3- and 4-bit tables of both curves on an MI355X.  The exponents'
    transform is zkp_ntt's (test_transform ties the two roots together), the points zkp_fixed_base_mul_g1's."""
    c = get_curve(curve)
    n = 1 << 17
    rng = random.Random(f"g1-ntt-{curve}-17")
    exps = [rng.randrange(c.r) for _ in range(n)]
    exps[n - 3] = 0
    xy, inf = device_points(ctx, c, curve, exps)
    want = device_points(ctx, c, curve, codec.fr_from_mont(ctx.ntt(c, codec.fr_to_mont(exps, c).reshape(n, 4), NTT_FFT), c))
    fwd = transform(ctx, c, xy, inf, NTT_FFT)
    assert same(fwd, want)
    assert same(transform(ctx, c, fwd[0], fwd[1], NTT_IFFT), (xy, inf))


# ------------------------------------------------------------------------------------------- argument rules
@pytest.mark.parametrize("curve", CURVES)
def test_argument_rules(ctx, curve):
    c = get_curve(curve)
    n, pb = 8, 16 * c.fq_limbs
    rng = random.Random(f"g1-ntt-args-{curve}")
    xy, inf = ref.points(curve, [rng.randrange(1, c.r) for _ in range(n)])
    sc = Framed(ctx, codec.fr_to_mont([rng.randrange(c.r) for _ in range(n)], c).reshape(n, 4), SENT)
    bx, bi = framed_points(ctx, xy, inf)
    ox, oi = framed_points(ctx, np.full_like(xy, SENT), np.full_like(inf, SENT_FLAG))
    lib, V = ctx.lib, C.c_void_p
    try:
        for log_n in (0, G1_NTT_MAX_LOG + 1):
            _bad(lambda: ctx.g1_ntt_dev(c, bx.ptr, bi.ptr, log_n, NTT_FFT))
        for op in (2, 3, -1):
            _bad(lambda: ctx.g1_ntt_dev(c, bx.ptr, bi.ptr, 3, op))
        _bad(lambda: ctx.g1_ntt_dev(c, bx.ptr + 8, bi.ptr, 2, NTT_FFT))              # misaligned points
        _bad(lambda: ctx.g1_ntt_dev(c, bx.ptr, bx.ptr + pb, 3, NTT_FFT))             # the flags inside the points
        _bad(lambda: ctx.g1_ntt_dev(c, 0, bi.ptr, 3, NTT_FFT))
        _bad(lambda: ctx.g1_ntt_dev(c, bx.ptr, 0, 3, NTT_FFT))                       # the flags are required
        assert lib.zkp_g1_ntt_dev(ctx.h, 7, V(bx.ptr), V(bi.ptr), 3, NTT_FFT) == -1  # a bad curve
        assert lib.zkp_g1_scale_vec_dev(ctx.h, 7, V(bx.ptr), V(bi.ptr), V(sc.ptr), n, V(ox.ptr), V(oi.ptr)) == -1
        _bad(lambda: ctx.g1_scale_vec_dev(c, bx.ptr, bi.ptr, sc.ptr + 8, n - 1, ox.ptr, oi.ptr))    # a misaligned scalar pointer
        _bad(lambda: ctx.g1_scale_vec_dev(c, bx.ptr + 8, bi.ptr, sc.ptr, n - 1, ox.ptr, oi.ptr))
        _bad(lambda: ctx.g1_scale_vec_dev(c, bx.ptr, bi.ptr, sc.ptr, n - 1, bx.ptr + pb, oi.ptr))   # partial overlap: points
        _bad(lambda: ctx.g1_scale_vec_dev(c, bx.ptr, bi.ptr, sc.ptr, n - 1, ox.ptr, bi.ptr + 1))    # partial overlap: flags
        _bad(lambda: ctx.g1_scale_vec_dev(c, bx.ptr, bi.ptr, sc.ptr, n, sc.ptr, oi.ptr))            # the output over the scalars
        _bad(lambda: ctx.g1_scale_vec_dev(c, bx.ptr, bi.ptr, sc.ptr, n, ox.ptr, ox.ptr + 16))       # the two outputs overlap
        for args in ((0, sc.ptr, ox.ptr, oi.ptr), (bx.ptr, 0, ox.ptr, oi.ptr), (bx.ptr, sc.ptr, 0, oi.ptr), (bx.ptr, sc.ptr, ox.ptr, 0)):
            _bad(lambda: ctx.g1_scale_vec_dev(c, args[0], bi.ptr, args[1], n, args[2], args[3]))
        ctx.sync()
        assert all(b.unchanged() for b in (sc, bx, bi, ox, oi)), "a rejected call wrote"
    finally:
        for b in (sc, bx, bi, ox, oi):
            b.free()
