"""zkp_fr_asvc_subset_weights_dev / zkp_fr_asvc_quotient_dev and ckb_zkp_amd.asvc on the device, bit-exact against tests/asvc_ref.py
(Python integers, long division).  Every writable buffer starts as sentinels with one sentinel element before and after it, whole
buffers are compared, and the inputs are read back unchanged.

The sizes sit on the kernel chain's boundaries: the segment length L = 2^floor(log2 k) (k = 1, 2, 3, 4, 5 ...), L against ASVC_SPAN
(k = 7, 8: the two forms of the output pass), the position group (ASVC_GROUP - 1 .. 2 ASVC_GROUP + 1), and n / L segments against
one and two scan chunks (32, 64 segments) and one and two scan tiles (2^13, 2^14 segments), and 2 ASVC_THREADS scan tiles (2^22
segments: the second window of the top scan; 1.8 s on an MI355X's host, nearly all of it the 2^22 steps of the Python recursion)."""
import random

import numpy as np
import pytest

from ckb_zkp_amd import _lib, asvc, codec
from ckb_zkp_amd.asvc import ASVC_CHUNK, ASVC_GROUP, ASVC_MAX_POSITIONS, ASVC_SPAN, ASVC_THREADS, ASVC_TILE
from ckb_zkp_amd.params import get_curve
from oracle.pyref.curves import Group
from tests import asvc_cases as cases
from tests import asvc_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xDEADBEEFCAFEF00D
G = ASVC_GROUP
GROUP_KS = [1, 2, G - 1, G, G + 1, 2 * G + 1]
SPAN_KS = [ASVC_SPAN - 1, ASVC_SPAN, 2 * ASVC_SPAN + 1]
assert ASVC_CHUNK == 32 and ASVC_TILE == 8192                     # the sizes below are poly.hip's, which the scan shares
PERIOD = 4099                                                     # the 2^22 input repeats a block of this (prime) length


def _bad(fn, status=-1):
    with pytest.raises(_lib.ZkpError) as e:
        fn()
    assert e.value.status == status


def positions(n, k, seed):
    """k distinct positions, unsorted, with 0, n / 2 (w = -1) and n - 1 among them where k allows"""
    rng = random.Random(seed)
    want = [n - 1, 0, n // 2]
    pts = []
    for p in want + rng.sample(range(n), min(n, k + 3)):
        if p not in pts and len(pts) < k:
            pts.append(p)
    if k > 3:
        rng.shuffle(pts)
    return pts


def phi_cases(c, n, points, seed, names):
    """name -> (coefficients, quotient or None (long division))"""
    rng = random.Random(seed)
    r, k = c.r, len(points)
    out = {}
    for name in names:
        if name == "random":
            out[name] = ([rng.randrange(r) for _ in range(n)], None)
        elif name == "zero":
            out[name] = ([0] * n, [0] * (n - k))
        elif name == "constant":
            out[name] = ([rng.randrange(1, r)] + [0] * (n - 1), [0] * (n - k))
        elif name == "top_half_zero":
            out[name] = ([rng.randrange(r) for _ in range(n // 2)] + [0] * (n - n // 2), None)
        elif name == "multiple":                                  # A_I times a random polynomial: remainder zero
            quo = [rng.randrange(r) for _ in range(n - k)]
            a = ref.vanishing(points, ref.domain_of(c.name, n).group_gen, r)
            out[name] = (ref.poly_mul(a, quo, r) if quo else [0] * n, quo)
        elif name == "rmax":                                      # the canonical maximum everywhere
            out[name] = ([r - 1] * n, None)
    return out


ALL_CASES = ["random", "zero", "constant", "top_half_zero", "multiple", "rmax"]


def device_quotient(ctx, c, phi, points):
    """runs the entry over sentinel-framed buffers; returns the n - k quotient words"""
    n, k = len(phi), len(points)
    words = codec.fr_to_mont(phi, c)
    sent = np.full((1, 4), SENT, dtype=np.uint64)
    host_in = np.concatenate([sent, words, sent])
    host_out = np.full((n - k + 2, 4), SENT, dtype=np.uint64)
    d_in, d_out = ctx.to_device(host_in), ctx.to_device(host_out)
    try:
        ctx.fr_asvc_quotient_dev(c, d_in + 32, n.bit_length() - 1, points, d_out + 32)
        got_in, got = np.zeros_like(host_in), np.zeros_like(host_out)
        ctx.d2h(got_in, d_in)
        ctx.d2h(got, d_out)
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
    assert np.array_equal(got_in, host_in), "the input changed"
    assert (got[0] == SENT).all() and (got[-1] == SENT).all(), "a write outside q"
    return got[1:-1]


def check_quotient(ctx, curve, n, k, names, seed):
    c = get_curve(curve)
    points = positions(n, k, seed)
    for name, (phi, quo) in phi_cases(c, n, points, seed + 1, names).items():
        if quo is None:
            quo = ref.quotient(curve, phi, points)
        assert len(quo) == n - k
        got = device_quotient(ctx, c, phi, points)
        assert np.array_equal(got, codec.fr_to_mont(quo, c).reshape(n - k, 4)), (curve, n, k, name)


# ------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("k", [1, 2, 3, 64, 65, 1024])
@pytest.mark.parametrize("curve", CURVES)
def test_weights(ctx, curve, k):
    c = get_curve(curve)
    log_n = 10
    points = positions(1 << log_n, k, k)
    want = codec.fr_to_mont(ref.subset_weights_direct(curve, 1 << log_n, points), c)
    if k <= 3:
        assert ref.subset_weights(curve, 1 << log_n, points) == ref.subset_weights_direct(curve, 1 << log_n, points)
    host = np.full((k + 2, 4), SENT, dtype=np.uint64)
    d = ctx.to_device(host)
    try:
        got_host = ctx.fr_asvc_subset_weights_dev(c, log_n, points, d + 32)
        got = np.zeros_like(host)
        ctx.d2h(got, d)
        assert np.array_equal(got_host, want)
        assert np.array_equal(got[1:-1], want) and (got[0] == SENT).all() and (got[-1] == SENT).all()
        # device output alone, host output alone
        ctx.h2d(d, host)
        assert ctx.fr_asvc_subset_weights_dev(c, log_n, points, d + 32, want_host=False) is None
        ctx.d2h(got, d)
        assert np.array_equal(got[1:-1], want)
        assert np.array_equal(ctx.fr_asvc_subset_weights_dev(c, log_n, points), want)
    finally:
        ctx.dev_free(d)
    if k == 1:
        assert codec.fr_from_mont(want, c) == [1]


# ------------------------------------------------------------------------------------------- quotient
@pytest.mark.parametrize("n", [2, 8, 32, 64])
@pytest.mark.parametrize("curve", CURVES)
def test_quotient_small_domains(ctx, curve, n):
    """one element, the reference's size, one and two scan chunks at k = 1; every k of the lists that fits, n - 1 and n"""
    for k in sorted({k for k in GROUP_KS + SPAN_KS + [n - 1, n] if 1 <= k <= n}):
        check_quotient(ctx, curve, n, k, ALL_CASES, 100 * n + k)


@pytest.mark.parametrize("log_n", [13, 14, 16])
@pytest.mark.parametrize("curve", CURVES)
def test_quotient_scan_tiles(ctx, curve, log_n):
    """one, two and several scan tiles at k = 1 (and the chunk / tile boundaries of the other segment lengths below them)"""
    n = 1 << log_n
    for k in GROUP_KS + SPAN_KS + ([33] if log_n == 16 else []):
        names = ALL_CASES if log_n == 13 and k in (1, G + 1) else ["random"] if k > 1 else ["random", "rmax"]
        check_quotient(ctx, curve, n, k, names, 1000 * log_n + k)


@pytest.mark.parametrize("n,k", [(1 << 11, 1023), (1 << 11, 1024), (1 << 12, 64), (1 << 12, 65), (1 << 10, 1024), (1 << 10, 1023)])
@pytest.mark.parametrize("curve", CURVES)
def test_quotient_many_positions(ctx, curve, n, k):
    """the cap and the segment lengths below it; Phi = A_I Q + R with deg R < k, so the quotient is Q by construction"""
    c = get_curve(curve)
    rng = random.Random(n + k)
    points = positions(n, k, n + k)
    quo = [rng.randrange(c.r) for _ in range(n - k)]
    a = ref.vanishing(points, ref.domain_of(curve, n).group_gen, c.r)
    phi = ref.poly_mul(a, quo, c.r) if quo else [0] * n
    phi = [(x + (rng.randrange(c.r) if t < k else 0)) % c.r for t, x in enumerate(phi + [0] * (n - len(phi)))]
    got = device_quotient(ctx, c, phi, points)
    assert np.array_equal(got, codec.fr_to_mont(quo, c).reshape(n - k, 4))


def test_quotient_two_windows_of_scan_tiles(ctx):
    """n = 2^22 at k = 1 (L = 1: every coefficient is a segment): 2 ASVC_THREADS scan tiles, the smallest domain at which
    asvc_scan_top_kernel takes a second window and the sum of the window above enters through `R * carry`.  The position is odd, so
    w has order n and r^TILE = w^TILE is no small root of unity: a wrong carry power changes the result.  The input repeats a block
    of prime length, encoded once and spread by indexing; the reference is q[t] = phi[t + 1] + w q[t + 1] on the Montgomery words
    themselves (the recursion is linear, so it holds for q R), which saves a second conversion of 2^22 elements.  The whole buffer is
    compared."""
    curve, log_n, p = "bn254", 22, 0x2AAAAB
    c = get_curve(curve)
    n, r = 1 << log_n, c.r
    assert n // ASVC_TILE == 2 * ASVC_THREADS and (n // 2) // ASVC_TILE <= ASVC_THREADS      # ntile: two windows here, one below
    assert p % 2 == 1 and 0 < p < n                                  # w = root^p has full order
    w = pow(ref.domain_of(curve, n).group_gen, p, r)
    assert pow(w, n // 2, r) == r - 1 and pow(w, ASVC_TILE * ASVC_THREADS, r) == r - 1
    rng = random.Random(22)
    base = [rng.randrange(r) for _ in range(PERIOD)]
    base[0], base[1] = 0, r - 1
    base_words = codec.fr_to_mont(base, c)
    base_m = codec.limbs_to_ints(base_words)                         # phi[t] R mod r
    sent = np.full((1, 4), SENT, dtype=np.uint64)
    host_in = np.concatenate([sent, base_words[np.arange(n) % PERIOD], sent])
    acc, raw = 0, [b""] * (n - 1)
    for t in range(n - 2, -1, -1):
        acc = (base_m[(t + 1) % PERIOD] + w * acc) % r
        raw[t] = acc.to_bytes(32, "little")
    want = np.full((n + 1, 4), SENT, dtype=np.uint64)
    want[1:-1] = np.frombuffer(b"".join(raw), dtype="<u8").reshape(n - 1, 4)
    del raw
    d_in, d_out = ctx.to_device(host_in), ctx.to_device(np.full((n + 1, 4), SENT, dtype=np.uint64))
    try:
        ctx.fr_asvc_quotient_dev(c, d_in + 32, log_n, [p], d_out + 32)
        got_in, got = np.zeros_like(host_in), np.zeros_like(want)
        ctx.d2h(got_in, d_in)
        ctx.d2h(got, d_out)
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
    assert np.array_equal(got_in, host_in), "the input changed"
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------- argument rules
@pytest.mark.parametrize("curve", CURVES)
def test_argument_rules(ctx, curve):
    c = get_curve(curve)
    log_n, n = 4, 16
    host = np.full((2 * n + 4, 4), SENT, dtype=np.uint64)
    d = ctx.to_device(host)
    phi, q = d + 32, d + 32 * (n + 2)
    lib, h = ctx.lib, ctx.h
    V = _lib.C.c_void_p

    def quot(phi_p=phi, log=log_n, pts=(1, 2, 3), q_p=q, k=None, cid=c.cid):
        pos = np.array(pts, dtype=np.uint32)
        _lib.check(lib.zkp_fr_asvc_quotient_dev(h, cid, V(phi_p), log, V(pos.ctypes.data), len(pos) if k is None else k, V(q_p)), "quotient")
        ctx.sync()

    def wts(log=log_n, pts=(1, 2, 3), out=q, host_out=True, k=None, cid=c.cid):
        pos = np.array(pts, dtype=np.uint32)
        buf = np.full((len(pos), 4), SENT, dtype=np.uint64)
        try:
            _lib.check(lib.zkp_fr_asvc_subset_weights_dev(h, cid, log, V(pos.ctypes.data), len(pos) if k is None else k, V(out),
                                                          V(buf.ctypes.data) if host_out else None), "weights")
        except _lib.ZkpError:
            assert (buf == SENT).all(), "the host output changed on an error"
            raise

    try:
        for fn in (quot, wts):
            _bad(lambda: fn(log=0))                                               # log_n >= 1
            _bad(lambda: fn(log=min(30, c.two_adicity) + 1), status=-3)           # above the limits of zkp_ntt_dev
            _bad(lambda: fn(cid=7), status=-2)                                    # no such curve
            _bad(lambda: fn(pts=(1, 2, 16)))                                      # a position >= n
            _bad(lambda: fn(pts=(1, 2, 1)))                                       # a repeated position
            _bad(lambda: fn(k=0))                                                 # k >= 1
            _bad(lambda: fn(pts=tuple(range(16)) + (3,)))                         # k > n
        _bad(lambda: quot(log=11, pts=tuple(range(ASVC_MAX_POSITIONS + 1))))      # above the cap (never read: the rule comes first)
        _bad(lambda: wts(log=11, pts=tuple(range(ASVC_MAX_POSITIONS + 1))))
        _bad(lambda: quot(phi_p=phi + 8))                                         # misaligned
        _bad(lambda: quot(q_p=q + 8))
        _bad(lambda: wts(out=q + 8))
        _bad(lambda: quot(q_p=phi))                                               # q over phi
        _bad(lambda: quot(q_p=phi + 32 * (n - 1)))                                # q starting on phi's last element
        _bad(lambda: quot(q_p=phi - 32 * (n - 3 - 1)))                            # q ending on phi's first element
        _bad(lambda: wts(out=0, host_out=False))                                  # no output at all
        got = np.zeros_like(host)
        ctx.d2h(got, d)
        assert np.array_equal(got, host), "an output changed on an error"
        # k == n: nothing is written, ZKP_OK
        quot(pts=tuple(range(16)))
        ctx.d2h(got, d)
        assert np.array_equal(got, host)
    finally:
        ctx.dev_free(d)


# ------------------------------------------------------------------------------------------- the driver
def _mont_g(c):
    oc = cases.inputs(c.name)[0]
    g1, g2 = cases.generators(oc)
    return codec.g1_to_mont([g1], c)[0][0], codec.g2_to_mont([g2], c)[0][0], g1, g2, oc


def _pt(c, p):
    """(xy, inf) -> the ref's affine point"""
    return codec.g1_from_mont(np.asarray(p[0]), [1 if p[1] else 0], c)[0]


@pytest.fixture(scope="module")
def keys(ctx):
    """the n = 8 key of the flow on the device, per curve, uploaded"""
    out = {}
    for curve in CURVES:
        c = get_curve(curve)
        g1m, g2m, _, _, _ = _mont_g(c)
        params = asvc.key_gen(ctx, c, cases.N, cases.TAU, g1m, g2m)
        params.proving_key.upload(ctx)
        out[curve] = params
    yield out
    for p in out.values():
        p.proving_key.free()


@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("curve", CURVES)
def test_key_gen(ctx, curve, n):
    c = get_curve(curve)
    g1m, g2m, g1, g2, oc = _mont_g(c)
    tau = cases.TAU + n
    params = asvc.key_gen(ctx, c, n - 1, tau, g1m, g2m)              # n - 1 is rounded up
    pk, vk = params.proving_key, params.verification_key
    assert pk.n == n
    _, powers, a_tau, a_s, l_s, u_s = ref.key_scalars(oc, n, tau)
    G1, G2 = Group(oc, 1), Group(oc, 2)
    flags = np.zeros(n + 1, dtype=np.uint8)
    assert codec.g1_from_mont(pk.powers_of_g1, flags, c) == [G1.mul(g1, s) for s in powers]
    assert codec.g2_from_mont(vk.powers_of_g2, flags, c) == [G2.mul(g2, s) for s in powers]
    assert codec.g1_from_mont(pk.a_i, flags, c) == [G1.mul(g1, s) for s in a_s]
    assert codec.g1_from_mont(pk.l_of_g1, flags, c) == [G1.mul(g1, s) for s in l_s]
    assert codec.g1_from_mont(pk.u_i, flags, c) == [G1.mul(g1, s) for s in u_s]
    assert codec.g1_from_mont(vk.a, [0], c) == [G1.mul(g1, a_tau)]
    with pytest.raises(ValueError):
        asvc.key_gen(ctx, c, n, pow(ref.domain_of(oc, n).group_gen, 3, c.r), g1m, g2m)     # tau in the domain


@pytest.mark.parametrize("curve", CURVES)
def test_flow_and_golden(ctx, keys, curve):
    c = get_curve(curve)
    oc, values, delta = cases.inputs(curve)
    golden = cases.golden_points(curve)
    js = cases.load_golden()[curve]
    assert [int(v, 16) for v in js["values"]] == values and int(js["tau"], 16) == cases.TAU and int(js["delta"], 16) == delta
    pk = keys[curve].proving_key
    n, i, j = cases.N, cases.UPDATE_INDEX, cases.OTHER_INDEX
    got = {"commit": asvc.commit(pk, values), "proof_015": asvc.prove_pos(pk, values, cases.PROVE_POINTS)}
    got["commit_updated"] = asvc.update_commit(ctx, c, got["commit"], delta, i, pk.update_key(i), n)
    got["proof_3"] = asvc.prove_pos(pk, values, [i])
    got["proof_3_updated"] = asvc.update_proof(ctx, c, got["proof_3"], delta, i, i, pk.update_key(i), pk.update_key(i), n)
    got["proof_4"] = asvc.prove_pos(pk, values, [j])
    got["proof_4_updated"] = asvc.update_proof(ctx, c, got["proof_4"], delta, j, i, pk.update_key(j), pk.update_key(i), n)
    got["proof_1"], got["proof_5"] = (asvc.prove_pos(pk, values, [p]) for p in cases.AGG_POINTS)
    got["aggregate_15"] = asvc.aggregate_proofs(ctx, c, n, cases.AGG_POINTS, [got["proof_1"], got["proof_5"]])
    assert {k: _pt(c, v) for k, v in got.items()} == golden
    # the ref's verifiers accept the device's proofs (the verification key from the device's key_gen)
    vkd = keys[curve].verification_key
    flags = np.zeros(n + 1, dtype=np.uint8)
    vk = ref.VerificationKey(codec.g1_from_mont(vkd.powers_of_g1, flags, c), codec.g2_from_mont(vkd.powers_of_g2, flags, c),
                             codec.g1_from_mont(vkd.a, [0], c)[0])
    w = ref.domain_of(oc, n).group_gen
    pts = cases.PROVE_POINTS
    assert ref.verify_pos(oc, vk, _pt(c, got["commit"]), [values[p] for p in pts], pts, _pt(c, got["proof_015"]), w)
    upk = pk.update_key(cases.UPK_INDEX)
    assert ref.verify_upk(oc, vk, cases.UPK_INDEX, ref.UpdateKey(_pt(c, (upk.ai, False)), _pt(c, (upk.ui, False))), w)
    # all n positions: the identity; rejected subsets
    assert asvc.prove_pos(pk, values, list(range(n)))[1] is True
    with pytest.raises(ValueError):
        asvc.prove_pos(pk, values, [1, 2, 1])
    with pytest.raises(ValueError):
        asvc.prove_pos(pk, values, list(range(ASVC_MAX_POSITIONS + 1)))
    stats = {}
    asvc.prove_pos(pk, values, pts, stats)
    assert set(stats) == {"upload", "ifft", "quotient", "msm", "affine"}


@pytest.mark.parametrize("m", [1, 2, 7])
@pytest.mark.parametrize("curve", CURVES)
def test_many_updates_equal_sequential_updates(ctx, keys, curve, m):
    c = get_curve(curve)
    _, values, _ = cases.inputs(curve)
    pk = keys[curve].proving_key
    n, own = cases.N, 2
    rng = random.Random(m)
    spots = [own, 5, 5, 0, 7, own, 3][:m] if m > 1 else [own]       # the proof's own position, one position twice
    changes = [(p, rng.randrange(1, c.r)) for p in spots]
    upks = [pk.update_key(p) for p, _ in changes]
    commitment, proof = asvc.commit(pk, values), asvc.prove_pos(pk, values, [own])
    seq_c, seq_p = commitment, proof
    for (p, d), u in zip(changes, upks):
        seq_c = asvc.update_commit(ctx, c, seq_c, d, p, u, n)
        seq_p = asvc.update_proof(ctx, c, seq_p, d, own, p, pk.update_key(own), u, n)
    many_c = asvc.update_commit_many(ctx, c, commitment, changes, upks, n)
    many_p = asvc.update_proof_many(ctx, c, proof, own, pk.update_key(own), changes, upks, n)
    assert _pt(c, many_c) == _pt(c, seq_c) and _pt(c, many_p) == _pt(c, seq_p)
    # and both equal a fresh commitment / proof of the changed vector
    new = list(values)
    for p, d in changes:
        new[p] = (new[p] + d) % c.r
    assert _pt(c, many_c) == _pt(c, asvc.commit(pk, new)) and _pt(c, many_p) == _pt(c, asvc.prove_pos(pk, new, [own]))


@pytest.mark.parametrize("curve", CURVES)
def test_aggregate_equals_prove_pos_of_the_subset(ctx, keys, curve):
    c = get_curve(curve)
    _, values, _ = cases.inputs(curve)
    pk = keys[curve].proving_key
    for subset in ([4], [6, 0], [7, 2, 4, 0, 5]):
        singles = [asvc.prove_pos(pk, values, [p]) for p in subset]
        assert _pt(c, asvc.aggregate_proofs(ctx, c, cases.N, subset, singles)) == _pt(c, asvc.prove_pos(pk, values, subset))


@pytest.mark.parametrize("curve", CURVES)
def test_prove_pos_two_scan_tiles(ctx, curve):
    """n = 2^14, k = 5 against [q(tau)] g1 formed in the exponent from tau (no Python MSM)"""
    c = get_curve(curve)
    g1m, _, g1, _, oc = _mont_g(c)
    n, points = 1 << 14, [n_ for n_ in (16383, 0, 8192, 77, 4099)]
    rng = random.Random(14)
    values = [rng.randrange(c.r) for _ in range(n - 3)]            # padded to n by prove_pos
    powers = codec.fr_canonical([pow(cases.TAU, j, c.r) for j in range(n + 1)], c)
    p1, _ = ctx.fixed_base_mul(c, 1, g1m, powers)
    pk = asvc.ProvingKey(c, n, p1, p1[:n], p1[:n], p1[:n]).upload(ctx)       # only powers_of_g1 is used
    try:
        got = asvc.prove_pos(pk, values, points)
    finally:
        pk.free()
    assert _pt(c, got) == ref.prove_pos_in_exponent(oc, n, cases.TAU, g1, values, points)
