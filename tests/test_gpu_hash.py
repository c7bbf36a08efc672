"""zkp_hash_params_* / zkp_fr_hash_blocks_dev / zkp_fr_hash_chain_dev / zkp_fr_mimc_trace_dev and ckb_zkp_amd.hashes on the device,
bit-exact against tests/hash_ref.py (Python integers).  Every buffer the device may write starts as sentinels with one sentinel
element before and after it, whole buffers are compared, and the inputs are read back unchanged.  The constants come from
circuits.prf_field_elements.

Sizes: one lane per block in workgroups of HASH_THREADS = 64, so n runs over 1, one workgroup less one, exactly one, one more, and
the same around four workgroups.  The reference of a parameter set is computed once, for the 257 inputs of the largest size; the
smaller sizes are its prefixes."""
import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec, hashes
from ckb_zkp_amd.circuits import prf_field_elements
from ckb_zkp_amd.params import get_curve
from tests import hash_cases as cases
from tests import hash_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xDEADBEEFCAFEF00D
NS = [1, 63, 64, 65, 255, 256, 257]
NMAX = max(NS)
assert hashes.HASH_THREADS == 64
V = _lib.C.c_void_p


def param_set(curve, name):
    if name == "mimc5":
        return cases.mimc_params(curve, 5)
    if name == "mimc322":
        return cases.mimc_params(curve, cases.REF_MIMC_ROUNDS)
    if name == "poseidon_ref":                                    # the reference's schedule: exactly one partial round
        return cases.poseidon_params(curve, hashes.poseidon_reference_schedule(cases.REF_POSEIDON_ROUNDS, cases.REF_POSEIDON_RF))
    if name == "poseidon_std":                                    # 4 full, 83 partial, 4 full
        return cases.poseidon_params(curve, hashes.poseidon_schedule(4, cases.REF_POSEIDON_RP, 4), seed=0x5EED)
    if name == "rescue22":
        return cases.rescue_params(curve, cases.REF_RESCUE_ROUNDS)
    if name == "rescue2":
        return cases.rescue_params(curve, 2)
    raise KeyError(name)


def first_constants(p):
    """what is added to (xl, xr) before the first S-box"""
    if p["kind"] == "mimc":
        return p["constants"][0], 0
    row = p["ark"][0] if p["kind"] == "poseidon" else p["constants"][0]
    return row[0], row[1]


def inputs(p, count, seed):
    """(xl, xr) lists: 0, r - 1, xl = -c_0 (t = 0 in MiMC, a zero state element before the first S-box elsewhere), xr = -c_1, both,
    then the PRF"""
    r = p["r"]
    c0, c1 = first_constants(p)
    vals = prf_field_elements(seed, 2 * count, r)
    xl, xr = vals[:count], vals[count:]
    special = [(0, 0), (r - 1, r - 1), (0, r - 1), (r - 1, 0), ((-c0) % r, 5), (7, (-c1) % r), ((-c0) % r, (-c1) % r), (1, 1)]
    for k, (a, b) in enumerate(special[:count]):
        xl[k], xr[k] = a, b
    return xl, xr


_SETS = {}


def uploaded(ctx, curve, name):
    """(parameter dict, HashParams, xl, xr, expected images) of one set, made once per session"""
    key = (curve, name)
    if key not in _SETS:
        p = param_set(curve, name)
        xl, xr = inputs(p, NMAX, 0xB10C + len(name))
        _SETS[key] = (p, cases.upload(ctx, curve, p), xl, xr, [ref.block(p, a, b) for a, b in zip(xl, xr)])
    return _SETS[key]


@pytest.fixture(scope="module", autouse=True)
def _free_sets():
    yield
    for _, hp, *_ in _SETS.values():
        hp.free()
    _SETS.clear()


def framed(words):
    sent = np.full((1, 4), SENT, dtype=np.uint64)
    return np.concatenate([sent, np.asarray(words, dtype=np.uint64).reshape(-1, 4), sent])


def sentinels(n):
    return np.full((n + 2, 4), SENT, dtype=np.uint64)


def read(ctx, ptr, like):
    got = np.zeros_like(like)
    ctx.d2h(got, ptr)
    return got


def run_blocks(ctx, c, hp, xl, xr, alias=None):
    """-> the n output words; alias: None (own buffer), "xl" or "xr" (the output is that input)"""
    n = len(xl)
    h_l, h_r, h_o = framed(codec.fr_to_mont(xl, c)), framed(codec.fr_to_mont(xr, c)), sentinels(n)
    d_l, d_r, d_o = ctx.to_device(h_l), ctx.to_device(h_r), ctx.to_device(h_o)
    try:
        out = {None: d_o, "xl": d_l, "xr": d_r}[alias]
        ctx.fr_hash_blocks_dev(hp.handle, d_l + 32, d_r + 32, n, out + 32)
        ctx.sync()
        g_l, g_r, g_o = read(ctx, d_l, h_l), read(ctx, d_r, h_r), read(ctx, d_o, h_o)
    finally:
        for d in (d_l, d_r, d_o):
            ctx.dev_free(d)
    got = {None: g_o, "xl": g_l, "xr": g_r}[alias]
    assert (got[0] == SENT).all() and (got[-1] == SENT).all(), "a write outside out"
    if alias != "xl":
        assert np.array_equal(g_l, h_l), "xl changed"
    if alias != "xr":
        assert np.array_equal(g_r, h_r), "xr changed"
    if alias is not None:
        assert np.array_equal(g_o, h_o), "the unused buffer changed"
    return got[1:-1]


# ------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", ["mimc5", "mimc322", "poseidon_ref", "poseidon_std", "rescue22"])
@pytest.mark.parametrize("curve", CURVES)
def test_blocks(ctx, curve, name, n):
    c = get_curve(curve)
    p, hp, xl, xr, want = uploaded(ctx, curve, name)
    got = run_blocks(ctx, c, hp, xl[:n], xr[:n])
    assert np.array_equal(got, codec.fr_to_mont(want[:n], c).reshape(n, 4)), (curve, name, n)
    if n == NMAX and name == "mimc5":
        # t = xl + c_0 = 0 in round 0: the round leaves (xr, xl)
        assert ref.mimc_block(xl[4], xr[4], p["constants"][:1], p["r"]) == xr[4]


@pytest.mark.parametrize("alias", ["xl", "xr"])
@pytest.mark.parametrize("name", ["mimc5", "poseidon_std", "rescue2"])
@pytest.mark.parametrize("curve", CURVES)
def test_blocks_in_place(ctx, curve, name, alias):
    c = get_curve(curve)
    n = 65
    _, hp, xl, xr, want = uploaded(ctx, curve, name)
    got = run_blocks(ctx, c, hp, xl[:n], xr[:n], alias=alias)
    assert np.array_equal(got, codec.fr_to_mont(want[:n], c).reshape(n, 4))


@pytest.mark.parametrize("alpha", [3, 7])
@pytest.mark.parametrize("curve", CURVES)
def test_other_exponents(ctx, curve, alpha):
    """alpha = 3 and 7: Poseidon always; Rescue where alpha is invertible mod r - 1 (3 divides r - 1 on both curves)"""
    c = get_curve(curve)
    n = 65
    sets = [cases.poseidon_params(curve, [1, 1, 0, 0, 1, 1], alpha=alpha)]
    if (c.r - 1) % alpha:
        sets.append(cases.rescue_params(curve, 2, alpha=alpha))
    assert alpha != 7 or len(sets) == 2
    for p in sets:
        hp = cases.upload(ctx, curve, p)
        try:
            assert hp.info()["alpha"] == alpha
            xl, xr = inputs(p, n, alpha)
            got = run_blocks(ctx, c, hp, xl, xr)
            assert np.array_equal(got, codec.fr_to_mont([ref.block(p, a, b) for a, b in zip(xl, xr)], c).reshape(n, 4)), p["kind"]
        finally:
            hp.free()


@pytest.mark.parametrize("curve", CURVES)
def test_rescue_inverse_sbox_of_zero(ctx, curve):
    """A matrix whose first row is zero and constants[1][0] = 0 leave state[0] = 0 in front of the first x^inv_alpha, for every
    input: 0^inv_alpha = 0 must come out of the square-and-multiply.  (An input with xl = -constants[0][0] only zeroes the state in
    front of the first x^alpha; test_blocks has it.)"""
    c = get_curve(curve)
    p = cases.rescue_params(curve, 2, seed=0x0)
    p["mds"][0] = [0, 0, 0]
    p["constants"][1][0] = 0
    hp = cases.upload(ctx, curve, p)
    try:
        n = 64
        xl, xr = inputs(p, n, 3)
        got = run_blocks(ctx, c, hp, xl, xr)
        assert np.array_equal(got, codec.fr_to_mont([ref.block(p, a, b) for a, b in zip(xl, xr)], c).reshape(n, 4))
    finally:
        hp.free()


# ------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("with_xl", [True, False])
@pytest.mark.parametrize("length", [1, 2, 5])
@pytest.mark.parametrize("name", ["mimc5", "poseidon_std", "rescue2"])
@pytest.mark.parametrize("curve", CURVES)
def test_chain(ctx, curve, name, length, with_xl):
    c = get_curve(curve)
    n = 65
    p, hp, *_ = uploaded(ctx, curve, name)
    vals = prf_field_elements(0xC4A1 + length, n * length, p["r"])
    vals[0], vals[1 % len(vals)] = 0, p["r"] - 1
    msgs = [vals[k * length:(k + 1) * length] for k in range(n)]
    triples = [ref.hash_elements(p, m) for m in msgs]
    h_m, h_o, h_x = framed(codec.fr_to_mont(vals, c)), sentinels(n), sentinels(n)
    d_m, d_o, d_x = ctx.to_device(h_m), ctx.to_device(h_o), ctx.to_device(h_x)
    try:
        ctx.fr_hash_chain_dev(hp.handle, d_m + 32, n, length, d_o + 32, d_x + 32 if with_xl else 0)
        ctx.sync()
        g_m, g_o, g_x = read(ctx, d_m, h_m), read(ctx, d_o, h_o), read(ctx, d_x, h_x)
    finally:
        for d in (d_m, d_o, d_x):
            ctx.dev_free(d)
    assert np.array_equal(g_m, h_m), "the messages changed"
    assert np.array_equal(g_o, framed(codec.fr_to_mont([t[2] for t in triples], c)))
    assert np.array_equal(g_x, framed(codec.fr_to_mont([t[0] for t in triples], c)) if with_xl else h_x)
    if length == 1:
        assert all(t[0] == 0 for t in triples)
    # the drivers
    if with_xl and length == 2:
        img, xls = hashes.hash_elements(hp, msgs[:3], want_xl=True)
        assert np.array_equal(img, g_o[1:4]) and np.array_equal(xls, g_x[1:4])
        data = b"".join(v.to_bytes(32, "little") for v in msgs[0]) + b"\x09"
        assert codec.fr_int(hashes.hash_bytes(hp, data), c) == ref.hash_elements(p, msgs[0] + [9])[2]


# ------------------------------------------------------------------------------------------- trace
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("rounds", [5, 322])
@pytest.mark.parametrize("curve", CURVES)
def test_mimc_trace(ctx, curve, rounds, extra):
    c = get_curve(curve)
    n = 65 if rounds == 5 else 64
    p, hp, xl, xr, _ = uploaded(ctx, curve, "mimc5" if rounds == 5 else "mimc322")
    xl, xr = xl[:n], xr[:n]
    row = 2 * rounds + 2
    stride = row + extra
    want = sentinels(n * stride)
    for k in range(n):
        want[1 + k * stride:1 + k * stride + row] = codec.fr_to_mont(ref.mimc_trace(xl[k], xr[k], p["constants"], p["r"]), c)
    h_l, h_r = framed(codec.fr_to_mont(xl, c)), framed(codec.fr_to_mont(xr, c))
    d_l, d_r, d_o = ctx.to_device(h_l), ctx.to_device(h_r), ctx.to_device(sentinels(n * stride))
    try:
        ctx.fr_mimc_trace_dev(hp.handle, d_l + 32, d_r + 32, n, d_o + 32, stride)
        ctx.sync()
        assert np.array_equal(read(ctx, d_o, want), want)              # the rows, the gaps between them, the frame
        assert np.array_equal(read(ctx, d_l, h_l), h_l) and np.array_equal(read(ctx, d_r, h_r), h_r)
    finally:
        for d in (d_l, d_r, d_o):
            ctx.dev_free(d)
    if extra == 0 and rounds == 5:
        got = hashes.mimc_trace(hp, xl[:3], xr[:3])
        assert np.array_equal(got.reshape(-1, 4), want[1:1 + 3 * row])
        assert np.array_equal(hashes.blocks(hp, xl[:3], xr[:3]), got[:, -1])


# ------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("curve", CURVES)
def test_params_info_and_creation_rules(ctx, curve):
    c = get_curve(curve)
    for name in ("mimc322", "poseidon_ref", "rescue22"):
        p, hp, *_ = uploaded(ctx, curve, name)
        info = hp.info()
        kind = {"mimc": 0, "poseidon": 1, "rescue": 2}[p["kind"]]
        rounds = {"mimc322": 322, "poseidon_ref": 91, "rescue22": 22}[name]
        assert (info["kind"], info["curve"], info["rounds"]) == (kind, c.cid, rounds)
        assert info["products"] == ref.products_of_block(p, hashes.HASH_RESCUE_WINDOW)
        n_consts = {"mimc322": 322, "poseidon_ref": 91 * 3 + 9, "rescue22": 45 * 3 + 9}[name]
        assert 32 * n_consts <= info["device_bytes"] <= 32 * n_consts + 4 * 130 + 8
    p = cases.rescue_params(curve, 2)
    one = codec.fr_to_mont([1], c)
    big = codec.ints_to_limbs([c.r], 4)                                # not canonical

    def create(kind=2, rounds=2, alpha=5, consts=None, mds=None, full=None, inv=p["inv_alpha"], size=None, cid=c.cid):
        consts = codec.fr_to_mont([x for row in p["constants"] for x in row], c) if consts is None else consts
        mds = codec.fr_to_mont([x for row in p["mds"] for x in row], c) if mds is None else mds
        full = np.ones(8, dtype=np.uint8) if full is None else full
        desc = _lib.HashDesc(_lib.C.sizeof(_lib.HashDesc) if size is None else size, kind, rounds, alpha, V(consts.ctypes.data),
                             V(mds.ctypes.data) if mds is not False else None, V(full.ctypes.data) if full is not False else None,
                             (_lib.C.c_uint64 * 4)(*[(inv >> (64 * i)) & (2**64 - 1) for i in range(4)]))
        out = V()
        st = ctx.lib.zkp_hash_params_create(ctx.h, cid, _lib.C.byref(desc), _lib.C.byref(out))
        if st == 0:
            ctx.hash_params_free(out.value)
        else:
            assert not out.value, "a handle came back with an error"
        return st

    assert create() == 0
    assert create(inv=p["inv_alpha"] + 1) == -1                        # the create-time check: (x^alpha)^inv != x
    assert create(inv=1) == -1 and create(inv=0) == -1
    assert create(kind=3) == -1 and create(kind=-1) == -1
    assert create(cid=7) == -2
    assert create(size=16) == -1 and create(size=0) == -1
    assert create(rounds=0) == -1 and create(rounds=hashes.HASH_MAX_ROUNDS_RESCUE + 1) == -1
    assert create(kind=1, rounds=hashes.HASH_MAX_ROUNDS_POSEIDON + 1) == -1 and create(kind=0, rounds=hashes.HASH_MAX_ROUNDS_MIMC + 1) == -1
    assert create(alpha=4) == -1 and create(alpha=0) == -1 and create(kind=1, alpha=9) == -1
    assert create(kind=0, alpha=0, mds=False, full=False) == 0         # MiMC needs neither
    assert create(mds=False) == -1 and create(kind=1, full=False) == -1 and create(kind=1) == 0
    bad = codec.fr_to_mont([x for row in p["constants"] for x in row], c)
    bad[-1] = big[0]
    assert create(consts=bad) == -1
    assert create(mds=np.concatenate([one] * 8 + [big])) == -1
    # a handle of another context
    from ckb_zkp_amd.api import Context
    _, hp, xl, xr, _ = uploaded(ctx, curve, "mimc5")
    other = Context(ctx.device)
    d = other.to_device(sentinels(6))
    try:
        with pytest.raises(_lib.ZkpError) as e:
            other.fr_hash_blocks_dev(hp.handle, d + 32, d + 64, 1, d + 96)
        assert e.value.status == -1
        with pytest.raises(_lib.ZkpError):
            other.hash_params_free(hp.handle)
        assert np.array_equal(read(other, d, sentinels(6)), sentinels(6))
    finally:
        other.dev_free(d)
        other.close()
    assert np.array_equal(run_blocks(ctx, c, hp, xl[:1], xr[:1]), codec.fr_to_mont([ref.block(param_set(curve, "mimc5"), xl[0], xr[0])], c))


# ------------------------------------------------------------------------------------------- argument rules
def _bad(fn, status=-1):
    with pytest.raises(_lib.ZkpError) as e:
        fn()
    assert e.value.status == status


@pytest.mark.parametrize("curve", CURVES)
def test_argument_rules(ctx, curve):
    _, mimc, *_ = uploaded(ctx, curve, "mimc5")
    _, pos, *_ = uploaded(ctx, curve, "poseidon_std")
    n, row = 4, 12
    host = sentinels(200)
    d = ctx.to_device(host)
    a, b, o, big = d + 32, d + 32 * 8, d + 32 * 16, d + 32 * 32        # a, b: n elements; o: n; big: up to 168
    try:
        blocks = lambda xl=a, xr=b, cnt=n, out=o, h=mimc.handle: ctx.fr_hash_blocks_dev(h, xl, xr, cnt, out)          # noqa: E731
        chain = lambda m=big, cnt=n, ln=3, out=o, x=a, h=pos.handle: ctx.fr_hash_chain_dev(h, m, cnt, ln, out, x)     # noqa: E731
        trace = lambda xl=a, xr=b, cnt=n, out=big, st=row, h=mimc.handle: ctx.fr_mimc_trace_dev(h, xl, xr, cnt, out, st)   # noqa: E731
        # NULL
        for kw in ({"xl": 0}, {"xr": 0}, {"out": 0}, {"h": 0}):
            _bad(lambda: blocks(**kw))
            _bad(lambda: trace(**kw))
        for kw in ({"m": 0}, {"out": 0}, {"h": 0}):
            _bad(lambda: chain(**kw))
        # misaligned
        for kw in ({"xl": a + 8}, {"xr": b + 8}, {"out": o + 8}):
            _bad(lambda: blocks(**kw))
        for kw in ({"m": big + 8}, {"out": o + 8}, {"x": a + 8}):
            _bad(lambda: chain(**kw))
        for kw in ({"xl": a + 8}, {"xr": b + 8}, {"out": big + 8}):
            _bad(lambda: trace(**kw))
        # counts
        cap = 1 << hashes.HASH_MAX_LOG_BLOCKS
        _bad(lambda: blocks(cnt=0))
        _bad(lambda: blocks(cnt=cap + 1))
        _bad(lambda: chain(cnt=0))
        _bad(lambda: chain(ln=0))
        _bad(lambda: chain(cnt=cap // 2 + 1, ln=2))
        _bad(lambda: chain(cnt=1, ln=cap + 1))
        _bad(lambda: trace(cnt=0))
        _bad(lambda: trace(cnt=cap + 1))
        _bad(lambda: trace(st=row - 1))                                                # a stride too small
        _bad(lambda: trace(cnt=1 << 20, st=(1 << 12) + 1))                             # n stride above 2^32
        _bad(lambda: trace(h=pos.handle))                                              # the trace is MiMC's
        # overlaps
        _bad(lambda: blocks(out=a + 32))                                               # out over xl, shifted by one element
        _bad(lambda: blocks(out=b - 32 * (n - 1)))                                     # out ending on xr's first element
        _bad(lambda: chain(out=big + 32 * 11))                                         # out on the last message element
        _bad(lambda: chain(x=o))                                                       # the two outputs on each other
        _bad(lambda: chain(x=o + 32 * (n - 1)))
        _bad(lambda: trace(out=a - 32 * (n * row - 1)))                                # the trace ending on xl's first element
        _bad(lambda: trace(xr=big + 32 * (n * row - 1)))                               # xr on the trace's last element
        ctx.sync()
        assert np.array_equal(read(ctx, d, host), host), "an output changed on an error"
    finally:
        ctx.dev_free(d)
