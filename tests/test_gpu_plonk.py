"""zkp_fr_prefix_product_dev / zkp_fr_plonk_perm_z_dev / zkp_fr_plonk_quotient_dev / ckb_zkp_amd.plonk on the device, bit-exact
against tests/plonk_ref.py (Python integers that follow plonk/src/composer, ahp/indexer and ahp/prover.rs).  Every output buffer
starts as sentinels with one sentinel element before and after it, and whole buffers are compared."""

import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec, plonk
from ckb_zkp_amd.params import get_curve
from ckb_zkp_amd.plonk import PLONK_QUOT_MAX_BLOCKS, PLONK_QUOT_THREADS, PLONK_SCAN_BLOCK
from tests import plonk_ref as ref
from tests.plonk_cases import KS, MINI_CHALLENGES, challenges, load_golden, mini_circuit, rand_fr, random_circuit

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xABABABABABABABAB
B = PLONK_SCAN_BLOCK
BAD_ARG, TOO_LARGE = -1, -3


class Bufs:
    """count buffers of n Fr side by side in one device allocation, a sentinel element before and after each"""

    def __init__(self, ctx, count, n):
        self.ctx, self.count, self.n = ctx, count, n
        self.host = np.full((count, n + 2, 4), SENT, dtype=np.uint64)
        self.dev = ctx.to_device(self.host)

    def ptr(self, i=0):
        return self.dev + 32 * ((self.n + 2) * i + 1)

    def fill(self, tables):
        """tables: count (n, 4) Montgomery arrays (None: sentinels)"""
        self.host[:] = SENT
        for i, t in enumerate(tables):
            if t is not None:
                self.host[i, 1:-1] = t
        self.ctx.h2d(self.dev, self.host)

    def read(self):
        out = np.zeros_like(self.host)
        self.ctx.d2h(out, self.dev)
        return out

    def expected(self, tables):
        exp = np.full_like(self.host, SENT)
        for i, t in enumerate(tables):
            if t is not None:
                exp[i, 1:-1] = t
        return exp

    def free(self):
        self.ctx.dev_free(self.dev)


def _status(fn, *args, **kw):
    with pytest.raises(_lib.ZkpError) as e:
        fn(*args, **kw)
    return e.value.status


def _mont(v, c):
    return codec.fr_to_mont(v, c)


# ------------------------------------------------------------------------------------------- running product
SCAN_SIZES = [1, 2, 3, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, B * B, B * B + 1, B * B + 2]
SCAN_MAX = max(SCAN_SIZES)


@pytest.fixture(scope="module")
def scan_data():
    """curve -> (input, exclusive running products and the total after each length), Montgomery limbs, for the longest size; a
    shorter size is a prefix of both.  The input repeats 4099 random elements (1 and r - 1 among them): the running product does
    not repeat.  Computed once, never modified."""
    out = {}
    for curve in CURVES:
        c = get_curve(curve)
        base = rand_fr(c.r, 4099, 31 + c.cid)
        base[1], base[2], base[70] = 1, c.r - 1, c.r - 1
        idx = np.arange(SCAN_MAX) % 4099
        R = 1 << 256
        acc, pref = R % c.r, []
        for i in idx.tolist():                                      # the Montgomery words themselves: acc R
            pref.append(acc)
            acc = acc * base[i] % c.r
        pref.append(acc)
        out[curve] = (_mont(base, c)[idx], codec.ints_to_limbs(pref, 4))
    return out


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_prefix_product(ctx, scan_data, curve, n):
    c = get_curve(curve)
    x, pref = scan_data[curve]
    x = x[:n]
    out = Bufs(ctx, 1, n)
    d_in = ctx.to_device(x)
    try:
        out.fill([None])                                             # out of place
        total = ctx.fr_prefix_product_dev(c, d_in, out.ptr(), n)
        assert np.array_equal(out.read(), out.expected([pref[:n]]))
        assert np.array_equal(total, pref[n])
        out.fill([x])                                                # in place, no total
        assert ctx.fr_prefix_product_dev(c, out.ptr(), out.ptr(), n, want_total=False) is None
        assert np.array_equal(out.read(), out.expected([pref[:n]]))
        if n >= 3:                                                   # a zero in the middle: everything after it is 0
            xz = x.copy()
            xz[n // 2] = 0
            exp = pref[:n].copy()
            exp[n // 2 + 1:] = 0
            for in_place in (False, True):
                out.fill([xz if in_place else None])
                ctx.h2d(d_in, xz)
                total = ctx.fr_prefix_product_dev(c, out.ptr() if in_place else d_in, out.ptr(), n)
                assert np.array_equal(out.read(), out.expected([exp])), in_place
                assert not total.any()
    finally:
        out.free()
        ctx.dev_free(d_in)


@pytest.mark.parametrize("curve", CURVES)
def test_prefix_product_rules(ctx, curve):
    c = get_curve(curve)
    buf = Bufs(ctx, 1, 64)
    try:
        buf.fill([_mont(rand_fr(c.r, 64, 5), c)])
        before = buf.read()
        p = buf.ptr()
        assert _status(ctx.fr_prefix_product_dev, c, p, p, 0) == BAD_ARG
        assert _status(ctx.fr_prefix_product_dev, c, p, p, (1 << 30) + 1) == BAD_ARG
        assert _status(ctx.fr_prefix_product_dev, c, p, p + 32, 8) == BAD_ARG          # overlap in part
        assert _status(ctx.fr_prefix_product_dev, c, p + 64, p, 8) == BAD_ARG
        assert _status(ctx.fr_prefix_product_dev, c, p + 8, p + 32 * 32, 8) == BAD_ARG  # misaligned
        ctx.fr_prefix_product_dev(c, p, p + 8 * 32, 8)                                  # disjoint halves are fine
        after = buf.read()
        assert np.array_equal(after[0, :9], before[0, :9]) and np.array_equal(after[0, 17:], before[0, 17:])
    finally:
        buf.free()


# ------------------------------------------------------------------------------------------- permutation accumulator
def _circuit(curve, log_n, seed):
    """a satisfied circuit whose domain is 2^log_n rows: (reference composer, selectors, witnesses)"""
    cs = ref.RefComposer(curve)
    if log_n == 3:
        mini_circuit(cs)
    else:
        random_circuit(cs, (1 << log_n) - (1 << log_n) // 8, seed)
    sel = cs.compose(KS)
    assert sel["n"] == 1 << log_n
    return cs, sel, cs.synthesize()


def _run_perm_z(ctx, c, log_n, w, sigma, beta, gamma, alias=False):
    """(z buffer as read back, expected buffer from the reference, closes, reference's closes)"""
    n = 1 << log_n
    ins = Bufs(ctx, 8, n)
    out = Bufs(ctx, 1, n)
    try:
        ins.fill([_mont(v, c) for v in list(w) + list(sigma)])
        out.fill([None])
        target = ins.ptr(1) if alias else out.ptr()
        closes = ctx.fr_plonk_perm_z_dev(c, [ins.ptr(j) for j in range(4)], [ins.ptr(4 + j) for j in range(4)], log_n, _mont(KS, c),
                                         codec.fr_mont(beta, c), codec.fr_mont(gamma, c), target)
        roots, x, g = [], 1, ref.Domain(ref.CURVES[c.name], n).group_gen
        for _ in range(n):
            roots.append(x)
            x = x * g % c.r
        z, ref_closes = ref.compute_z(w, sigma, roots, KS, beta, gamma, c.r)
        if alias:
            got, exp = ins.read(), ins.expected([_mont(v, c) for v in list(w) + list(sigma)])
            exp[1, 1:-1] = _mont(z, c)
        else:
            got, exp = out.read(), out.expected([_mont(z, c)])
            assert np.array_equal(ins.read(), ins.expected([_mont(v, c) for v in list(w) + list(sigma)]))   # inputs untouched
        return got, exp, closes, ref_closes
    finally:
        ins.free()
        out.free()


# 2: the smallest domain; 3: the mini circuit; 10 / 11: one workgroup (n == PLONK_SCAN_BLOCK) and two; 13: 8 blocks and their scan
@pytest.mark.parametrize("log_n", [2, 3, 10, 11, 13])
@pytest.mark.parametrize("curve", CURVES)
def test_perm_z(ctx, curve, log_n):
    c = get_curve(curve)
    assert (1 << 10) == B
    _, sel, w = _circuit(curve, log_n, 40 + log_n)
    sigma = [sel[s] for s in ref.S_NAMES]
    beta, gamma, _ = challenges(c.r, log_n)
    got, exp, closes, ref_closes = _run_perm_z(ctx, c, log_n, w, sigma, beta, gamma)
    assert ref_closes and closes
    assert np.array_equal(got, exp)
    # one witness value changed: the accumulator no longer closes, z is still the running product
    bad = [list(col) for col in w]
    bad[2][(1 << log_n) // 3] = (bad[2][(1 << log_n) // 3] + 1) % c.r
    got, exp, closes, ref_closes = _run_perm_z(ctx, c, log_n, bad, sigma, beta, gamma)
    assert not ref_closes and not closes
    assert np.array_equal(got, exp)
    # a zero denominator in row n / 2: 1 / 0 = 0, z is 0 from the next row on, the call returns normally
    i = (1 << log_n) // 2
    zero = [list(col) for col in w]
    zero[0][i] = -(beta * sigma[0][i] + gamma) % c.r
    got, exp, closes, ref_closes = _run_perm_z(ctx, c, log_n, zero, sigma, beta, gamma)
    assert not closes and not ref_closes
    assert not exp[0, i + 2:-1].any() and exp[0, i + 1].any()
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("curve", CURVES)
def test_perm_z_may_overwrite_an_input_and_rules(ctx, curve):
    c = get_curve(curve)
    log_n = 4
    _, sel, w = _circuit(curve, log_n, 3)
    sigma = [sel[s] for s in ref.S_NAMES]
    beta, gamma, _ = challenges(c.r, 9)
    got, exp, closes, _ = _run_perm_z(ctx, c, log_n, w, sigma, beta, gamma, alias=True)
    assert closes and np.array_equal(got, exp)
    buf = Bufs(ctx, 9, 16)
    try:
        buf.fill([_mont(rand_fr(c.r, 16, k), c) for k in range(9)])
        before = buf.read()
        wp, sp, zp = [buf.ptr(j) for j in range(4)], [buf.ptr(4 + j) for j in range(4)], buf.ptr(8)
        ks, one = _mont(KS, c), codec.fr_mont(1, c)
        r_words = codec.ints_to_limbs([c.r], 4)[0]
        run = ctx.fr_plonk_perm_z_dev
        assert _status(run, c, wp, sp, 1, ks, one, one, zp) == BAD_ARG
        assert _status(run, c, wp, sp, c.two_adicity - 1, ks, one, one, zp) == TOO_LARGE
        assert _status(run, c, wp, sp, 4, ks, r_words, one, zp) == BAD_ARG
        assert _status(run, c, wp, sp, 4, ks, one, r_words, zp) == BAD_ARG
        assert _status(run, c, wp, sp, 4, np.stack([one, one, r_words, one]), one, one, zp) == BAD_ARG
        assert _status(run, c, wp[:3] + [wp[3] + 8], sp, 4, ks, one, one, zp) == BAD_ARG
        assert _status(run, c, wp, sp, 4, ks, one, one, zp + 8) == BAD_ARG
        assert np.array_equal(buf.read(), before)                    # nothing ran
    finally:
        buf.free()


# ------------------------------------------------------------------------------------------- quotient
TABLES = ["w_0", "w_1", "w_2", "w_3", "z", "pi"] + list(ref.Q_NAMES) + list(ref.S_NAMES) + ["l1"]


def _quotient_call(ctx, c, ins, log_n, beta, gamma, alpha, t_ptr):
    at = {name: ins.ptr(k) for k, name in enumerate(TABLES)}
    ctx.fr_plonk_quotient_dev(c, [at[f"w_{j}"] for j in range(4)], at["z"], at["pi"], [at[q] for q in ref.Q_NAMES],
                              [at[s] for s in ref.S_NAMES], at["l1"], log_n, _mont(KS, c), codec.fr_mont(beta, c), codec.fr_mont(gamma, c),
                              codec.fr_mont(alpha, c), t_ptr)


# 2: 16 points, the last four read z[0..4); 11: 8192 points in 32 workgroups
@pytest.mark.parametrize("log_n", [2, 3, 6, 11])
@pytest.mark.parametrize("curve", CURVES)
def test_quotient(ctx, curve, log_n):
    """uniformly random tables (the formula is pointwise: they need not come from a circuit), so z_4n has no period"""
    c = get_curve(curve)
    N = 4 << log_n
    t = {name: rand_fr(c.r, N, 100 * log_n + k) for k, name in enumerate(TABLES)}
    for k in range(0, N, 5):
        t["q_arith"][k] = 0                                          # the is_zero() branch of arithmetic.rs:104
    t["q_arith"][1] = c.r - 1
    for k, name in enumerate(TABLES):                                # operands 0 and r - 1 in every table, on different rows
        t[name][(2 * k) % N] = 0
        t[name][(2 * k + 7) % N] = c.r - 1
    t["z"][N - 1], t["z"][0], t["z"][3] = c.r - 1, 0, 1
    beta, gamma, alpha = challenges(c.r, 50 + log_n)
    exp = ref.quotient_pointwise(t, ref.coset_points(curve, log_n), ref.v_4n_inversed(curve, log_n), KS, beta, gamma, alpha, c.r)
    ins, out = Bufs(ctx, len(TABLES), N), Bufs(ctx, 1, N)
    try:
        tables = [_mont(t[name], c) for name in TABLES]
        ins.fill(tables)
        out.fill([None])
        _quotient_call(ctx, c, ins, log_n, beta, gamma, alpha, out.ptr())
        assert np.array_equal(out.read(), out.expected([_mont(exp, c)]))
        assert np.array_equal(ins.read(), ins.expected(tables))
    finally:
        ins.free()
        out.free()


@pytest.mark.parametrize("curve", CURVES)
def test_quotient_beyond_one_grid(ctx, curve):
    """4n = 2^18 points: twice the kernel's PLONK_QUOT_THREADS * PLONK_QUOT_MAX_BLOCKS threads, so every thread takes a second point
    with x stepped by w^T.  Every table repeats 1000 random rows (the stride between a thread's points is no multiple of 1000);
    x_i = g w^i, the row z[(i + 4) mod 4n] across the wrap and 1 / (x_i^n - 1) do not repeat, so the reference computes the
    repeating factors once per row of the base and everything that depends on i per point (arrays of Python integers)."""
    c = get_curve(curve)
    r = c.r
    log_n = 16
    N, P = 4 << log_n, 1000
    assert N == 2 * PLONK_QUOT_THREADS * PLONK_QUOT_MAX_BLOCKS
    base = {name: rand_fr(r, P, 900 + k) for k, name in enumerate(TABLES)}
    for k in range(0, P, 5):
        base["q_arith"][k] = 0
    beta, gamma, alpha = challenges(r, 77)
    idx = np.arange(N) % P
    o = lambda v: np.array(v, dtype=object)                           # noqa: E731
    b = {k: o(v) for k, v in base.items()}
    d = ref.Domain(ref.CURVES[curve], N)
    xs = o([d.coset_gen])
    while len(xs) < N:                                               # x_i = g w^i by doubling
        xs = np.concatenate([xs, xs * pow(d.group_gen, len(xs), r) % r])
    arith = (b["q_0"] * b["w_0"] + b["q_1"] * b["w_1"] + b["q_2"] * b["w_2"] + b["q_3"] * b["w_3"] + b["q_m"] * b["w_1"] * b["w_2"]
             + b["q_c"] + b["pi"]) * b["q_arith"] % r
    rest = (arith + (b["z"] - 1) * b["l1"] * (alpha * alpha % r)) % r
    den = o([1] * P)
    for j in range(4):
        den = den * ((b[f"w_{j}"] + beta * b[f"sigma_{j}"] + gamma) % r) % r
    z = b["z"][idx]
    num = z
    for j in range(4):
        num = num * (((b[f"w_{j}"] + gamma) % r)[idx] + (KS[j] * beta % r) * xs) % r
    den = den[idx] * z[(np.arange(N) + 4) % N] % r
    vinv = o(ref.v_4n_inversed_four(curve, log_n)[:4])[np.arange(N) % 4]
    exp = ((num - den) * alpha + rest[idx]) % r * vinv % r
    exp = codec.ints_to_limbs((exp * ((1 << 256) % r) % r).tolist(), 4)
    ins, out = Bufs(ctx, len(TABLES), N), Bufs(ctx, 1, N)
    try:
        ins.fill([_mont(base[name], c)[idx] for name in TABLES])
        out.fill([None])
        _quotient_call(ctx, c, ins, log_n, beta, gamma, alpha, out.ptr())
        assert np.array_equal(out.read(), out.expected([exp]))
    finally:
        ins.free()
        out.free()


@pytest.mark.parametrize("curve", CURVES)
def test_quotient_rejects_an_aliased_output_and_bad_arguments(ctx, curve):
    c = get_curve(curve)
    log_n, N = 2, 16
    ins = Bufs(ctx, len(TABLES) + 1, N)
    try:
        ins.fill([_mont(rand_fr(c.r, N, k), c) for k in range(len(TABLES) + 1)])
        before = ins.read()
        beta, gamma, alpha = challenges(c.r, 1)
        for k in range(len(TABLES)):                                 # t_out on every input in turn, and overlapping it in part
            assert _status(_quotient_call, ctx, c, ins, log_n, beta, gamma, alpha, ins.ptr(k)) == BAD_ARG, TABLES[k]
        assert _status(_quotient_call, ctx, c, ins, log_n, beta, gamma, alpha, ins.ptr(len(TABLES) - 1) + 32 * 8) == BAD_ARG
        assert _status(_quotient_call, ctx, c, ins, log_n, beta, gamma, alpha, ins.ptr(len(TABLES)) + 8) == BAD_ARG   # misaligned
        assert _status(_quotient_call, ctx, c, ins, 1, beta, gamma, alpha, ins.ptr(len(TABLES))) == BAD_ARG
        assert _status(_quotient_call, ctx, c, ins, c.two_adicity - 1, beta, gamma, alpha, ins.ptr(len(TABLES))) == TOO_LARGE
        at = [ins.ptr(k) for k in range(len(TABLES))]
        one, r_words = codec.fr_mont(1, c), codec.ints_to_limbs([c.r], 4)[0]
        for bad in range(3):
            sc = [one, one, one]
            sc[bad] = r_words
            assert _status(ctx.fr_plonk_quotient_dev, c, at[0:4], at[4], at[5], at[6:13], at[13:17], at[17], log_n, _mont(KS, c), *sc,
                           ins.ptr(len(TABLES))) == BAD_ARG
        assert np.array_equal(ins.read(), before)                    # nothing ran
    finally:
        ins.free()


# ------------------------------------------------------------------------------------------- driver
def _drive(ctx, curve, build, beta, gamma, alpha):
    """rounds 1-3 of ckb_zkp_amd.plonk for the circuit build(composer): (reference index, reference composer, device polys)"""
    cs = build(plonk.Composer(curve))
    ix = plonk.Index(ctx, curve, cs.compose(KS), KS)
    ps = None
    try:
        ps = plonk.prover_init(ix, cs.public_inputs())
        polys = dict(zip(("w_0", "w_1", "w_2", "w_3"), plonk.prover_first_round(ps, cs.synthesize())))
        polys["z"] = plonk.prover_second_round(ps, beta, gamma)
        polys.update(zip(("t_0", "t_1", "t_2", "t_3"), plonk.prover_third_round(ps, alpha)))
    finally:
        if ps:
            ps.close()
        ix.close()
    return polys


@pytest.mark.parametrize("kind", ["mini", "random"])
@pytest.mark.parametrize("curve", CURVES)
def test_driver_rounds(ctx, curve, kind):
    c = get_curve(curve)
    build = mini_circuit if kind == "mini" else (lambda cs: random_circuit(cs, 1000, 11))
    ch = (MINI_CHALLENGES["beta"], MINI_CHALLENGES["gamma"], MINI_CHALLENGES["alpha"]) if kind == "mini" else challenges(c.r, 21)
    polys = _drive(ctx, curve, build, *ch)
    rcs = build(ref.RefComposer(curve))
    rix = ref.RefIndex(rcs, KS)
    assert rix.n == (8 if kind == "mini" else 1024)
    exp = ref.prove_rounds(rix, rcs.synthesize(), rcs.public_inputs(), *ch)
    assert exp["closes"]
    for name, v in polys.items():
        assert v == exp[name], name
    if kind == "mini" and curve == "bls12_381":
        gold = load_golden()
        for name in ("z", "t_0", "t_1", "t_2", "t_3"):
            assert polys[name] == gold[name], name
    zeta = rand_fr(c.r, 1, 5)[0]
    lhs, rhs = ref.round3_identity(rix, polys, rcs.public_inputs(), *ch, zeta)       # on the device's output
    assert lhs == rhs


@pytest.mark.parametrize("curve", CURVES)
def test_driver_frees_its_buffers_and_reports_a_bad_witness(ctx, curve, monkeypatch):
    c = get_curve(curve)
    live = set()
    alloc, free = ctx.dev_alloc, ctx.dev_free

    def counting_alloc(nbytes):
        p = alloc(nbytes)
        live.add(p)
        return p

    def counting_free(p):
        live.remove(p)
        free(p)

    monkeypatch.setattr(ctx, "dev_alloc", counting_alloc)
    monkeypatch.setattr(ctx, "dev_free", counting_free)
    beta, gamma, alpha = challenges(c.r, 2)
    for cycle in range(2):                                           # a second build-and-close cycle on the same context
        cs = mini_circuit(plonk.Composer(curve))
        ix = plonk.Index(ctx, curve, cs.compose(KS), KS)
        assert len(ix.bufs) == 11 + 4 + 1 and len(live) == 16
        ps = plonk.prover_init(ix, cs.public_inputs())
        w = cs.synthesize()
        w[1][0] = (w[1][0] + 1) % c.r                                # gate 0's left wire no longer equals gate 1's
        plonk.prover_first_round(ps, w, to_host=False)
        with pytest.raises(ValueError, match="does not close"):
            plonk.prover_second_round(ps, beta, gamma)
        plonk.prover_first_round(ps, cs.synthesize(), to_host=False)
        plonk.prover_second_round(ps, beta, gamma, to_host=False)
        plonk.prover_third_round(ps, alpha, to_host=False)
        ps.close()
        ix.close()
        assert not live and ix.bufs == [] and ps.bufs == []
        ix.close()                                                   # closing twice is harmless
