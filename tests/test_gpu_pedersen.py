"""zkp_pedersen_key_* / zkp_pedersen_commit_rows_dev on the device, bit-exact against Python integers over oracle.pyref.curves.

Every generator of a test key is a known multiple a_j of the group generator, so the reference of one row is ONE scalar
multiplication, (sum_j s_j a_j + blind a_h) G, whatever cols is; the outputs are canonical affine, so they are compared bit for bit.
Equal generators (a_1 = a_0), opposite ones (a_1 = r - a_0), identities (a_j = 0) and h = g_0 are such keys too.  Every writable
buffer starts as sentinels with one sentinel element before and after it, whole buffers are compared, and the inputs are read back
unchanged.  G (generators per slice) and c come from zkp_pedersen_key_info, so the shapes follow the plan: one slice, one slice
exactly, two and three slices; 63 / 64 / 65 rows are the batch of the affine pass.

Rows of more slices than the row pass has lanes (test_row_pass_second_trip: 64, 65 and 66 slices) and the key cap (test_key_cap:
65536 generators, 529 slices) use keys that repeat PERIOD of the base points.  Measured on an MI355X: a case of
test_row_pass_second_trip takes 0.04 - 0.2 s (its two keys 0.4 s once), test_key_cap 0.14 s."""
import functools
import random

import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec
from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.polycommit import PEDERSEN_MAX_GENS, PEDERSEN_ROW_LANES
from oracle.pyref.curves import Group
from tests.util import OC

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xDEADBEEFCAFEF00D
ROWS = [1, 2, 63, 64, 65]
MAX_GENS, MAX_CELLS = 65536, 1 << 28
G_PLAN, C_PLAN = 124, 8                  # what zkp_pedersen_key_info reports (asserted below): sizes the shared key before a context exists
NG = 2 * G_PLAN + 2                      # generators of the shared key: every cols below is < n_gens
LANES = PEDERSEN_ROW_LANES               # lane t of the row pass adds slices t, t + LANES, ... of its row
LONG_COLS = [LANES * G_PLAN, LANES * G_PLAN + 1, (LANES + 1) * G_PLAN + 1]       # one slice per lane; lane 0, lanes 0 and 1 take a second
PERIOD = 64                              # of the long keys' generators: no multiple or divisor of G_PLAN, LANES g is a multiple of it


def _bad(fn, status=-1):
    with pytest.raises(_lib.ZkpError) as e:
        fn()
    assert e.value.status == status


@functools.lru_cache(maxsize=None)
def base_exps(curve):
    rng = random.Random("pedersen " + curve)
    r = get_curve(curve).r
    return tuple(rng.randrange(1, r) for _ in range(NG + 1))      # a_0 .. a_{NG-1}, then a_h


@functools.lru_cache(maxsize=None)
def point_of(curve, a):
    gp = Group(OC[curve], 1)
    return gp.mul(gp.gen, a) if a % gp.order else None


class Key:
    """a device key whose generators are exps[j] G (0: the identity) and whose h is h_exp G"""

    def __init__(self, ctx, curve, exps, h_exp, flag_identities=True):
        self.ctx, self.c, self.exps, self.h_exp = ctx, get_curve(curve), list(exps), h_exp
        xy, inf = codec.g1_to_mont([point_of(curve, a) for a in exps], self.c)
        hxy, _ = codec.g1_to_mont([point_of(curve, h_exp)], self.c)
        self.h = ctx.pedersen_key_create(self.c, xy, inf if flag_identities else None, hxy[0])
        self.info = ctx.pedersen_key_info(self.h)

    def free(self):
        self.ctx.pedersen_key_free(self.h)

    def expected(self, scalars, blinds):
        r = self.c.r
        pts = []
        for i, row in enumerate(scalars):
            e = sum(s * a for s, a in zip(row, self.exps)) + (blinds[i] * self.h_exp if blinds is not None else 0)
            pts.append(point_of(self.c.name, e % r))
        return codec.g1_to_mont(pts, self.c)


@pytest.fixture(scope="module")
def keys(ctx):
    made = {}

    def get(curve):
        if curve not in made:
            e = base_exps(curve)
            made[curve] = Key(ctx, curve, e[:NG], e[NG])
            info = made[curve].info
            assert info["n_gens"] == NG and info["c"] == C_PLAN and info["gens_per_slice"] == G_PLAN and info["launches"] == 3
            assert info["W"] * info["c"] > 256 and info["pairs_per_slice"] <= 4096 and info["lds_bytes"] <= 160 * 1024
            w = 2 * made[curve].c.fq_limbs
            assert info["table_bytes"] == info["W"] * (NG + 1) * w * 8
        return made[curve]
    yield get
    for k in made.values():
        k.free()


def commit(key, scalars, blinds):
    """runs the entry over sentinel-framed buffers; returns (xy, inf) of the rows"""
    ctx, c = key.ctx, key.c
    rows, cols, w = len(scalars), len(scalars[0]), 2 * c.fq_limbs
    sent = np.full((1, 4), SENT, dtype=np.uint64)
    h_s = np.concatenate([sent, codec.fr_to_mont([s for row in scalars for s in row], c), sent])
    h_b = None if blinds is None else np.concatenate([sent, codec.fr_to_mont(blinds, c), sent])
    h_xy = np.full(2 * 2 + rows * w, SENT, dtype=np.uint64)          # 16 bytes of sentinels on either side
    h_inf = np.full(rows + 32, 0xA5, dtype=np.uint8)
    bufs = [ctx.to_device(a) for a in (h_s, h_xy, h_inf)] + ([] if h_b is None else [ctx.to_device(h_b)])
    try:
        ctx.pedersen_commit_rows_dev(key.h, bufs[0] + 32, rows, cols, None if h_b is None else bufs[3] + 32, bufs[1] + 16, bufs[2] + 16)
        g_s, g_xy, g_inf = np.zeros_like(h_s), np.zeros_like(h_xy), np.zeros_like(h_inf)
        ctx.d2h(g_s, bufs[0])
        ctx.d2h(g_xy, bufs[1])
        ctx.d2h(g_inf, bufs[2])
        if h_b is not None:
            g_b = np.zeros_like(h_b)
            ctx.d2h(g_b, bufs[3])
            assert np.array_equal(g_b, h_b), "the blinds changed"
    finally:
        for p in bufs:
            ctx.dev_free(p)
    assert np.array_equal(g_s, h_s), "the scalars changed"
    assert (g_xy[:2] == SENT).all() and (g_xy[-2:] == SENT).all(), "a write outside out_xy"
    assert (g_inf[:16] == 0xA5).all() and (g_inf[-16:] == 0xA5).all(), "a write outside out_inf"
    return g_xy[2:-2].reshape(rows, w), g_inf[16:-16]


def check(key, scalars, blinds, what):
    xy, inf = commit(key, scalars, blinds)
    want_xy, want_inf = key.expected(scalars, blinds)
    assert np.array_equal(inf, want_inf), what
    assert np.array_equal(xy, want_xy), what


def edge_scalars(r, c):
    """name -> scalar: the window digits of DigitIter at their boundaries (windows are c = 8 bits: one byte each)"""
    assert c == 8
    half = 1 << (c - 1)
    rep = lambda b, top=0: int.from_bytes(bytes([b] * 31 + [top]), "little")
    out = {"zero": 0, "one": 1, "r-1": r - 1,
           "plus_half": rep(half),                # every digit +2^(c-1): the largest bucket, no carry
           "minus_half_plus_1": rep(half + 1),    # 2^(c-1) + 1: the first negative digit, -(2^(c-1) - 1), with a carry
           "half_minus_1": rep(half - 1, 0),      # below the boundary
           "all_negative": rep(0xC0),             # every window but the top one negative; the top digit is the last carry
           "carry_chain": rep(0xFF, 0x0F)}        # 0xff + carry = 2^c: a zero digit that still carries
    assert all(0 <= v < r for v in out.values())
    return out


@pytest.mark.parametrize("cols", [1, 2, 3, G_PLAN - 1, G_PLAN, G_PLAN + 1, 2 * G_PLAN + 1])
@pytest.mark.parametrize("curve", CURVES)
def test_shapes(keys, curve, cols):
    key = keys(curve)
    rng = random.Random(f"{curve} {cols}")
    r = key.c.r
    for k, rows in enumerate(ROWS):
        scalars = [[rng.randrange(r) for _ in range(cols)] for _ in range(rows)]
        blinds = [rng.randrange(r) for _ in range(rows)] if (k + cols) % 2 else None
        check(key, scalars, blinds, (curve, rows, cols, blinds is not None))
    # both forms at the shape that is not covered by the alternation above
    scalars = [[rng.randrange(r) for _ in range(cols)] for _ in range(2)]
    check(key, scalars, [rng.randrange(r), 0], (curve, 2, cols, "blind and zero blind"))
    check(key, scalars, None, (curve, 2, cols, "no blinds"))


@pytest.mark.parametrize("curve", CURVES)
def test_scalar_patterns(keys, curve):
    key = keys(curve)
    r, cols = key.c.r, G_PLAN + 1
    rng = random.Random("patterns " + curve)
    edges = edge_scalars(r, key.info["c"])
    rows, names = [], []
    for name, v in edges.items():                                    # all equal: one bucket per window
        rows.append([v] * cols)
        names.append(name)
    vals = list(edges.values())
    rows.append([vals[j % len(vals)] for j in range(cols)])          # 0, 1, r - 1 and the boundary digits side by side
    rows.append([rng.choice([0, 1, r - 1]) for _ in range(cols)])
    rows.append([rng.randrange(r) for _ in range(cols)])
    blinds = [vals[i % len(vals)] for i in range(len(rows))]
    check(key, rows, blinds, (curve, "patterns with blinds", names))
    check(key, rows, None, (curve, "patterns", names))
    xy, inf = commit(key, [[0] * cols] * 3, [0, 0, 0])               # all zero: the identity, written as zkp_fixed_base_mul_g1 does
    assert (inf == 1).all() and (xy == 0).all()
    one_xy, one_inf = key.ctx.fixed_base_mul(key.c, 1, codec.g1_to_mont([point_of(curve, 1)], key.c)[0][0], codec.fr_canonical([0], key.c))
    assert np.array_equal(one_xy[0], xy[0]) and one_inf[0] == inf[0]


# ------------------------------------------------------------------------------------------- rows of more slices than lanes
def periodic_exps(curve, n):
    """n generator exponents that repeat the first PERIOD known-dlog base points: no new point_of call, whatever n is"""
    e = base_exps(curve)
    return [e[j % PERIOD] for j in range(n)]


@pytest.fixture(scope="module")
def long_keys(ctx):
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = Key(ctx, curve, periodic_exps(curve, LONG_COLS[-1]), base_exps(curve)[NG])
        return made[curve]
    yield get
    for k in made.values():
        k.free()


def row_plan(key, cols):
    """(S, g) of pedersen_plan from the G the key reports"""
    G = key.info["gens_per_slice"]
    S = -(-cols // G)
    return S, -(-cols // S)


@pytest.mark.parametrize("cols", LONG_COLS)
@pytest.mark.parametrize("curve", CURVES)
def test_row_pass_second_trip(long_keys, curve, cols):
    """ped_row_kernel's lane t adds slices t, t + LANES, ...: LANES G columns are the last shape of one slice per lane, one column
    more gives lane 0 a second slice (the plan balances the slices, so S = LANES + 1 slices of g < G generators, the last one
    shorter), (LANES + 1) G + 1 columns give lanes 0 and 1 one.  The key repeats PERIOD base points (periodic_exps), so the reference
    of a row stays one scalar multiplication.  A slice holds more than PERIOD generators, so points repeat inside it and enter one
    bucket twice whenever their digits agree: always in the row whose scalars are all equal, where the bucket sums meet additions of
    equal points.  That is kept on purpose.  In that row at (LANES + 1) G + 1 columns slices 0 and LANES hold the same generators
    (LANES g is a multiple of PERIOD) and return the same point, so lane 0's second addition is a doubling."""
    key = long_keys(curve)
    G, r = key.info["gens_per_slice"], key.c.r
    assert G == G_PLAN and G % PERIOD and PERIOD % G and key.info["n_gens"] == LONG_COLS[-1] >= cols
    S, g = row_plan(key, cols)
    assert S == {LANES * G: LANES, LANES * G + 1: LANES + 1, (LANES + 1) * G + 1: LANES + 2}[cols]
    assert (S > LANES) == (cols > LANES * G) and (S - 1) * g < cols <= S * g <= S * G and g > PERIOD
    if cols == LONG_COLS[-1]:                                       # slice LANES is a whole slice over the generators of slice 0
        assert (LANES * g) % PERIOD == 0 and (LANES + 1) * g <= cols
    rng = random.Random(f"long {curve} {cols}")
    equal = [rng.randrange(1, r)] * cols
    one = [[rng.randrange(r) for _ in range(cols)]]
    check(key, one, [rng.randrange(r)], (curve, 1, cols, "blind"))
    check(key, one, None, (curve, 1, cols, "no blind"))
    two = [[rng.randrange(r) for _ in range(cols)], equal]
    check(key, two, [rng.randrange(r), rng.randrange(r)], (curve, 2, cols, "blinds"))
    check(key, two, None, (curve, 2, cols, "no blinds"))
    check(key, [equal], None, (curve, 1, cols, "all equal"))


def test_key_cap(ctx):
    """n_gens = cols = PED_MAX_GENS on BN254: S = 529 slices, eight or nine per lane of the row pass, and 1025 workgroups per level
    of key creation; one row with a blind.  The table (about 138 MB) is freed whatever happens."""
    curve = "bn254"
    c = get_curve(curve)
    key = Key(ctx, curve, periodic_exps(curve, MAX_GENS), base_exps(curve)[NG])
    try:
        info = key.info
        assert info["n_gens"] == MAX_GENS == PEDERSEN_MAX_GENS and info["gens_per_slice"] == G_PLAN and info["launches"] == 3
        assert info["table_bytes"] == info["W"] * (MAX_GENS + 1) * 2 * c.fq_limbs * 8
        S, g = row_plan(key, MAX_GENS)
        assert S > 8 * LANES and (S - 1) * g < MAX_GENS <= S * g <= S * G_PLAN
        assert -(-(MAX_GENS + 1) // LANES) == MAX_GENS // LANES + 1 > 1024       # workgroups of a level of key creation
        rng = random.Random("cap")
        check(key, [[rng.randrange(c.r) for _ in range(MAX_GENS)]], [rng.randrange(1, c.r)], (curve, "cap"))
    finally:
        key.free()


@pytest.mark.parametrize("variant", ["equal", "opposite", "flagged_identity", "zero_words_identity", "h_is_g0", "h_identity"])
@pytest.mark.parametrize("curve", CURVES)
def test_special_keys(ctx, curve, variant):
    e = list(base_exps(curve))
    r = get_curve(curve).r
    exps, h_exp, flag = e[:5], e[NG], True
    if variant == "equal":
        exps[1] = exps[0]
    elif variant == "opposite":
        exps[1] = r - exps[0]
    elif variant == "flagged_identity":
        exps[2] = 0
    elif variant == "zero_words_identity":
        exps[0], flag = 0, False
    elif variant == "h_is_g0":
        h_exp = exps[0]
    elif variant == "h_identity":
        h_exp = 0
    key = Key(ctx, curve, exps, h_exp, flag)
    try:
        rng = random.Random(variant + curve)
        s0 = rng.randrange(1, r)
        rows = [[rng.randrange(r) for _ in range(5)] for _ in range(3)]
        rows += [[s0, s0, 0, 0, 0], [s0, r - s0, 0, 0, 0], [1, 1, 1, 1, 1], [s0, 0, 0, 0, 0]]
        blinds = [rng.randrange(r) for _ in range(6)] + [r - s0]     # last row with h = g_0: s_0 g_0 + (r - s_0) g_0, the identity
        check(key, rows, blinds, (curve, variant, "blinds"))
        check(key, rows, None, (curve, variant))
        check(key, [[s0], [1], [0]], [r - s0, r - 1, 0], (curve, variant, "cols = 1"))
        if variant == "h_is_g0":
            xy, inf = commit(key, [[s0]], [r - s0])
            assert inf[0] == 1 and (xy == 0).all()
        if variant == "opposite":
            xy, inf = commit(key, [[s0, s0, 0, 0, 0]], None)
            assert inf[0] == 1 and (xy == 0).all()
    finally:
        key.free()


@pytest.mark.parametrize("curve", CURVES)
def test_argument_rules_write_nothing(ctx, keys, curve):
    key = keys(curve)
    c, w = key.c, 2 * key.c.fq_limbs
    rows, cols = 2, 3
    h_s = codec.fr_to_mont(list(range(1, rows * cols + 1)), c)
    h_big = np.full((64, 4), SENT, dtype=np.uint64)                 # scalars, blinds and out_xy candidates with room to shift
    h_inf = np.full(64, 0xA5, dtype=np.uint8)
    d_s, d_b, d_xy, d_inf = ctx.to_device(h_s), ctx.to_device(h_big), ctx.to_device(h_big), ctx.to_device(h_inf)
    try:
        run = lambda **kw: ctx.pedersen_commit_rows_dev(kw.get("key", key.h), kw.get("s", d_s), kw.get("rows", rows), kw.get("cols", cols),
                                                        kw.get("b", d_b), kw.get("xy", d_xy), kw.get("inf", d_inf))
        for name in ("key", "s", "xy", "inf"):                       # NULL pointers (blinds may be NULL)
            _bad(lambda: run(**{name: 0}))
        for name, p in (("s", d_s), ("b", d_b), ("xy", d_xy)):       # misaligned pointers
            _bad(lambda: run(**{name: p + 8}))
        _bad(lambda: run(cols=NG + 1))
        _bad(lambda: run(cols=0))
        _bad(lambda: run(rows=0))
        _bad(lambda: run(rows=MAX_CELLS // cols + 1))                # rows * cols over the cap
        _bad(lambda: run(xy=d_s))                                    # an output over an input
        _bad(lambda: run(xy=d_b))
        _bad(lambda: run(inf=d_s + 8))
        _bad(lambda: run(inf=d_xy + 8))                              # one output inside the other
        _bad(lambda: run(xy=d_xy + 16 * 8, inf=d_xy + 16 * 8 + rows * w * 8 - 1))
        got_big, got_inf, got_s = np.zeros_like(h_big), np.zeros_like(h_inf), np.zeros_like(h_s)
        for d in (d_b, d_xy):
            ctx.d2h(got_big, d)
            assert np.array_equal(got_big, h_big), "a refused call wrote"
        ctx.d2h(got_inf, d_inf)
        ctx.d2h(got_s, d_s)
        assert np.array_equal(got_inf, h_inf) and np.array_equal(got_s, h_s), "a refused call wrote"
        run(b=0)                                                     # the same buffers are accepted once the rules hold
    finally:
        for d in (d_s, d_b, d_xy, d_inf):
            ctx.dev_free(d)
    # key creation: n_gens 0 or over the cap, NULL points
    one = codec.g1_to_mont([point_of(curve, 1)], c)[0]
    _bad(lambda: ctx.pedersen_key_create(c, np.zeros((0, w), dtype=np.uint64), None, one[0]))
    _bad(lambda: ctx.pedersen_key_create(c, np.zeros((MAX_GENS + 1, w), dtype=np.uint64), None, one[0]))
    handle = _lib.C.c_void_p()
    assert ctx.lib.zkp_pedersen_key_create(ctx.h, c.cid, None, None, 1, one.ctypes.data, _lib.C.byref(handle)) == -1
    assert ctx.lib.zkp_pedersen_key_create(ctx.h, c.cid, one.ctypes.data, None, 1, None, _lib.C.byref(handle)) == -1
    assert ctx.lib.zkp_pedersen_key_create(ctx.h, c.cid, one.ctypes.data, None, 1, one.ctypes.data, None) == -1
    assert handle.value is None
    _bad(lambda: ctx.pedersen_key_free(0))
    _bad(lambda: ctx.pedersen_key_info(0))
