"""Every MSM window plan, sort path and reduction variant, in-process and at small sizes.

msm_run_entry (csrc/msm.hip: the phases of MsmRun, sized by csrc/msm_sort_plan.hpp) picks between many kernel paths by the
public window bits / chunk size / table budget of zkp_ctx_config and by the internal switches of csrc/tune.hpp.  Each case below is ONE context created under one such setting
(latched at creation; the environment is clean again before anything is uploaded), and every (curve, group) runs inside it:

  * the plan the library prints at upload (ZKP_DEBUG_MSM, read live by bases_upload; the context itself latched it as 0) must equal
    the plain-integer model of tests/msm_plan_ref.py;
  * an EDGE set of 48 bases d_i G (an identity base, a duplicate pair and a P, -P pair with equal scalars) with the scalars
    0, 1, 2, r - 1, r - 2, (r - 1) / 2, the model's two "every digit at / one above the sign change" scalars and 2^j, 2^j - 1 at
    window boundaries of the plan under test, at six (n, offset); 48 bases hold 14 boundaries, so the plan's other boundaries
    follow, 14 at a time, in further MSMs over the same uploaded bases until EVERY boundary has run;
  * a MULTI-TILE set of 2 * 2048 + 513 bases: three level-1 sort tiles, the last a quarter full and ending inside a staged
    sub-round; 301 equal scalars (a 301-entry bucket, more than 32 tasks once the task cap is 4), a tenth zeros, 50 ones.

Expectations are (sum d_i k_i mod r) G in Python integers and the oracle's group law; the default plan's result on the same input
is compared as an extra.  Nothing starts a process."""
import contextlib
import functools
import random
import re

import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec
from ckb_zkp_amd.params import get_curve
from oracle.pyref.curves import Group
from tests import msm_plan_ref as M
from tests import util
from tests.util import OC, jac_limbs_to_affine_oracle, random_points, to_abi_points

pytestmark = pytest.mark.gpu
CFG = [("bn254", 1), ("bn254", 2), ("bls12_381", 1), ("bls12_381", 2)]
G1 = [("bn254", 1), ("bls12_381", 1)]
PLAN_RE = re.compile(r"\[msm\] bases group=(\d+) n=(\d+): c=(\d+) W=(\d+) wide=(\d+) k=(\d+) copies=(\d+)")
N_EDGE, N_MULTI = 48, 2 * 2048 + 513
EDGE_CASES = [(48, 0), (1, 0), (0, 0), (17, 5), (60, 0), (3, 47)]            # (scalars, offset): 60 overruns the bases, (3, 47) leaves one
MULTI_CASES = [(N_MULTI, 0), (2049, 2560), (2048, 1)]
N_BOUNDS = 14                                                                 # window boundaries an edge set has room for


@pytest.fixture
def variant_ctx(monkeypatch):
    """variant_ctx(device, config, env): tests.util.variant_ctx on this test's monkeypatch"""
    return functools.partial(util.variant_ctx, monkeypatch)


class Inputs:
    """The input sets of one (curve, group), built once with the session context, and their expectations."""

    def __init__(self, ctx, curve, group):
        self.ctx, self.curve, self.group = ctx, curve, group
        self.c = c = get_curve(curve)
        self.G = G = Group(OC[curve], group)
        self.g_xy, _ = to_abi_points(curve, group, [G.gen])
        self.points, self.exp, self.default, self.default_bases = {0: None}, {}, {}, None
        rnd = random.Random(1000 * group + len(curve))
        r = c.r
        # edge set: d_6 = 0 (an identity base), d_7 = d_8 (a duplicate pair), d_10 = -d_9 (P, -P)
        d = [rnd.randrange(1, r) for _ in range(N_EDGE)]
        d[6], d[8], d[10] = 0, d[7], r - d[9]
        self.edge_d = d
        self.edge_xy, self.edge_inf = ctx.fixed_base_mul(c, group, self.g_xy, codec.fr_canonical(d, c))
        assert self.edge_inf.tolist() == [int(i == 6) for i in range(N_EDGE)]
        for i in (0, 10, N_EDGE - 1):                                          # the device built them: three against the oracle
            assert np.array_equal(self.edge_xy[i], to_abi_points(curve, group, [G.mul(G.gen, d[i])])[0][0]), i
        self.edge_fill = [rnd.randrange(r) for _ in range(60)]
        # multi-tile set
        rng = np.random.default_rng(77 * group + len(curve))
        dm = rng.integers(0, 1 << 63, size=(N_MULTI, 4), dtype=np.uint64)
        dm[:, 3] >>= np.uint64(4)                                              # < 2^251 < r
        dm[7] = 0                                                              # an identity base
        self.multi_d = codec.limbs_to_ints(dm)
        self.multi_xy, self.multi_inf = ctx.fixed_base_mul(c, group, self.g_xy, dm)
        assert self.multi_inf[7] == 1 and self.multi_inf.sum() == 1
        for i in (0, N_MULTI - 1):
            assert np.array_equal(self.multi_xy[i], to_abi_points(curve, group, [G.mul(G.gen, self.multi_d[i])])[0][0]), i
        ku = [int.from_bytes(rng.bytes(40), "little") % r for _ in range(N_MULTI)]          # uniform in [0, r)
        self.uniform_k = ku
        self.uniform = codec.fr_canonical(ku, c).reshape(-1, 4)
        km = list(ku)
        km[1000:1300] = [km[999]] * 300                                        # 300 equal scalars in a row (and km[999]: 301)
        for i in np.flatnonzero(rng.random(N_MULTI) < 0.1):
            if not 999 <= i < 1300:
                km[i] = 0
        for i in rng.choice(np.arange(1300, N_MULTI), size=50, replace=False):
            km[i] = 1
        self.multi_k = km
        self.multi = codec.fr_canonical(km, c).reshape(-1, 4)
        self._mont = None

    def point(self, e):
        """e G by the oracle (cached: most variants share their expectations)"""
        e %= self.c.r
        if e not in self.points:
            self.points[e] = self.G.mul(self.G.gen, e)
        return self.points[e]

    def dot(self, d, k, n, off):
        m = max(0, min(n, len(d) - off))
        return self.point(sum(a * b for a, b in zip(d[off:off + m], k[:m])))

    def multi_exp(self, n, off, uniform=False):
        key = (n, off, uniform)
        if key not in self.exp:
            self.exp[key] = self.dot(self.multi_d, self.uniform_k if uniform else self.multi_k, n, off)
        return self.exp[key]

    def multi_default(self, n, off):
        """the session context's (default plan, unchunked below 3 * 2^20 points) result on the multi-tile set"""
        if (n, off) not in self.default:
            if self.default_bases is None:
                self.default_bases = self.ctx.upload_bases(self.c, self.group, self.multi_xy, self.multi_inf)
            self.default[(n, off)] = affine(self, self.default_bases.msm(self.multi[:n], off))
        return self.default[(n, off)]

    def multi_mont(self):
        if self._mont is None:
            self._mont = codec.fr_to_mont(self.multi_k, self.c).reshape(-1, 4)
        return self._mont

    def free(self):
        if self.default_bases is not None:
            self.default_bases.free()


@pytest.fixture(scope="module")
def inputs(ctx):
    sets = {}

    def get(curve, group):
        if (curve, group) not in sets:
            sets[(curve, group)] = Inputs(ctx, curve, group)
        return sets[(curve, group)]
    yield get
    for s in sets.values():
        s.free()


def affine(I, out):
    return jac_limbs_to_affine_oracle(I.curve, I.group, out)


def model_plan(curve, group, n, config, env, lgk=None):
    """what bases_upload must print for a stand-alone base vector in a context of (config, env): (group, n, c, W, wide, k, copies)"""
    if lgk is None:
        lgk = M.table_lgk(int(env["ZKP_TABLE_K"])) if "ZKP_TABLE_K" in env else 0
    c, W, wide, lgk, J = M.window_plan(M.SCALAR_BITS[curve], n, group, 0, lgk, env.get("ZKP_MSM_BALANCED", 1) != 0, lone=True,
                                       msm_c=config.get("msm_window_bits", 0), msm_c_g2=config.get("msm_window_bits_g2", 0),
                                       widen=env.get("ZKP_MSM_WIDEN", 1) != 0)
    return (group, n, c, W, wide, 1 << lgk, J)


@contextlib.contextmanager
def uploaded(v, capfd, monkeypatch, I, xy, inf, want_plan):
    """bases in the variant context (the plan is fixed at upload), the printed plan held against the model, freed on exit"""
    capfd.readouterr()
    monkeypatch.setenv("ZKP_DEBUG_MSM", "1")                   # live for the upload's print only: the context latched 0
    try:
        b = v.upload_bases(I.c, I.group, xy, inf)
    finally:
        monkeypatch.delenv("ZKP_DEBUG_MSM")
    try:
        printed = [tuple(int(x) for x in m) for m in PLAN_RE.findall(capfd.readouterr().err)]
        assert printed == [want_plan], (I.curve, I.group)
        yield b
    finally:
        b.free()


def boundary_passes(I, plan):
    """EVERY window boundary j of the plan with 2^j < r, in passes of N_BOUNDS: the scalars of an MSM are not fixed at upload, so
    the boundaries an edge set has no room for go into further MSMs over the same uploaded bases"""
    _, _, c, W, wide, _, _ = plan
    b = [j for j in M.window_positions(c, W, wide)[1:] if j <= M.SCALAR_BITS[I.curve] - 1]
    assert len(b) >= W - 2
    return [b[i:i + N_BOUNDS] for i in range(0, len(b), N_BOUNDS)]


def edge_scalars(I, plan, bounds):
    _, _, c, W, wide, _, _ = plan
    r = I.c.r
    ks = list(I.edge_fill)
    ks[0:6] = 0, 1, 2, r - 1, r - 2, (r - 1) // 2
    ks[8], ks[10] = ks[7], ks[9]                               # the duplicate pair and P, -P meet in every bucket
    ks[11], ks[12] = M.threshold_scalars(c, W, wide, M.SCALAR_BITS[I.curve])
    for i, j in enumerate(bounds):
        ks[13 + 2 * i], ks[14 + 2 * i] = 1 << j, (1 << j) - 1
    assert len(bounds) <= N_BOUNDS and all(0 <= k < r for k in ks)
    return ks


def check_edge(v, capfd, monkeypatch, I, config, env, lgk=None):
    plan = model_plan(I.curve, I.group, N_EDGE, config, env, lgk)
    passes = boundary_passes(I, plan)
    with uploaded(v, capfd, monkeypatch, I, I.edge_xy, I.edge_inf, plan) as b:
        for p, bounds in enumerate(passes):
            ks = edge_scalars(I, plan, bounds)
            for n, off in EDGE_CASES if p == 0 else EDGE_CASES[:1]:      # the further passes differ in slots 13 .. 40 only
                got = affine(I, b.msm(codec.fr_canonical(ks[:n], I.c).reshape(-1, 4), off))
                assert got == I.dot(I.edge_d, ks, n, off), (I.curve, I.group, plan, n, off, bounds)


def multi_cases(b, I, plan):
    for n, off in MULTI_CASES:
        got = affine(I, b.msm(I.multi[:n], off))
        assert got == I.multi_exp(n, off), (I.curve, I.group, plan, n, off)
        assert got == I.multi_default(n, off), (I.curve, I.group, plan, n, off)


def check_multi(v, capfd, monkeypatch, I, config, env, lgk=None):
    plan = model_plan(I.curve, I.group, N_MULTI, config, env, lgk)
    with uploaded(v, capfd, monkeypatch, I, I.multi_xy, I.multi_inf, plan) as b:
        multi_cases(b, I, plan)


def run_both_sets(variant_ctx, inputs, capfd, monkeypatch, config, env, lgk=None, cfgs=CFG):
    with variant_ctx(inputs("bn254", 1).ctx.device, config, env) as v:
        for curve, group in cfgs:
            I = inputs(curve, group)
            check_edge(v, capfd, monkeypatch, I, config, env, lgk)
            check_multi(v, capfd, monkeypatch, I, config, env, lgk)


def bits(c):
    return dict(msm_window_bits=c, msm_window_bits_g2=c)


def ids(variants):
    return [",".join(f"{k.replace('ZKP_', '').replace('msm_window_bits', 'c')}={v}" for d in x[:2] for k, v in d.items()
                     if k != "msm_window_bits_g2") or "default" for x in variants]


# ------------------------------------------------------------------------------------------- A, B: window bits, equal widths
@pytest.mark.parametrize("c", [2, 3, 4, 5, 11, 12, 13, 14, 20, 21, 22])
def test_window_bits(variant_ctx, inputs, capfd, monkeypatch, c):
    """A: msm_window_bits = msm_window_bits_g2 = c.  2: 128 windows, two buckets, the top window of a 255-bit T one bit wide;
    11 -> 12: the bucket id outgrows the 10 level-1 bits; 12 -> 13: 2^(c-1) reaches PAIR_TOP_MAX; 22: 2^21 buckets, level-2 bins
    of 2^11 keys; 21 needs 13 windows, which balance to 20 and 19 bits — the plan of 20."""
    run_both_sets(variant_ctx, inputs, capfd, monkeypatch, bits(c), {})


def test_window_bits_of_g2_bases_are_their_own(variant_ctx, inputs, capfd, monkeypatch):
    """A: msm_window_bits_g2 governs G2 bases and msm_window_bits the G1 bases of the same context (12 and 5 bits)."""
    config = dict(msm_window_bits=12, msm_window_bits_g2=5)
    assert [model_plan("bn254", g, N_EDGE, config, {})[2:4] for g in (1, 2)] == [(12, 22), (5, 51)]
    run_both_sets(variant_ctx, inputs, capfd, monkeypatch, config, {})


@pytest.mark.parametrize("c", [2, 7, 13, 20, 22])
def test_equal_window_widths(variant_ctx, inputs, capfd, monkeypatch, c):
    """B: ZKP_MSM_BALANCED=0: W windows of c bits, the top one thin and reaching past bit 255."""
    run_both_sets(variant_ctx, inputs, capfd, monkeypatch, bits(c), {"ZKP_MSM_BALANCED": 0})


# ------------------------------------------------------------------------------------------- C: the default rule
@pytest.mark.parametrize("widen", [1, 0])
def test_default_window_rule(variant_ctx, inputs, capfd, monkeypatch, widen):
    """C: no configured bits; the printed c follows the model at the clamp (16 -> 4), on both sides of sqrt(2) 2^9 and sqrt(2) 2^10,
    at 2^10 - 1 and 2^10 (+ 3 with widening) and at the multi-tile size; uniform scalars against slices of the multi-tile bases."""
    env = {} if widen else {"ZKP_MSM_WIDEN": 0}
    want_c = {1: {16: 4, 724: 9, 725: 13, 1023: 13, 1024: 13, 1448: 13, 1449: 14, N_MULTI: 15},
              0: {16: 4, 724: 9, 725: 10, 1023: 10, 1024: 10, 1448: 10, 1449: 11, N_MULTI: 12}}[widen]
    with variant_ctx(inputs("bn254", 1).ctx.device, {}, env) as v:
        for curve, group in CFG:
            I = inputs(curve, group)
            T = M.SCALAR_BITS[curve] + 1
            for n, c0 in want_c.items():
                plan = model_plan(curve, group, n, {}, env)
                assert plan[2] == -(-T // -(-T // c0)), (n, plan)        # the rule's c0 (written out above), balanced over ceil(T / c0) windows
                with uploaded(v, capfd, monkeypatch, I, I.multi_xy[:n], I.multi_inf[:n], plan) as b:
                    assert len(I.uniform[:n]) == n
                    assert affine(I, b.msm(I.uniform[:n])) == I.multi_exp(n, 0, uniform=True), (curve, group, n)
                    if n == N_MULTI:
                        multi_cases(b, I, plan)                      # and the multi-tile scalars against the session context's result


# ------------------------------------------------------------------------------------------- D: window groups
GROUPS = [({}, {"ZKP_TABLE_K": k}) for k in (2, 4, 8, 16, 64)] + [(bits(5), {"ZKP_TABLE_K": k}) for k in (4, 16)]


@pytest.mark.parametrize("config,env", GROUPS, ids=ids(GROUPS))
def test_window_groups(variant_ctx, inputs, capfd, monkeypatch, config, env):
    """D: k consecutive windows share one table copy and use k bucket sets; k >= W collapses to one copy; 5 configured bits
    with k = 4 / 16 hit the max(4, c0 - lgk) clamp."""
    run_both_sets(variant_ctx, inputs, capfd, monkeypatch, config, env)


def test_window_groups_by_a_table_budget_nothing_fits(variant_ctx, inputs, capfd, monkeypatch):
    """D: table_budget_gb = 1e-6 (1073 bytes) is less than ONE copy of 48 points: the planner ends at its largest group size, 64,
    which is one copy for every plan here — a correct result, not an error."""
    config = dict(table_budget_gb=1e-6)
    for curve, group in CFG:
        for n in (N_EDGE, N_MULTI):
            assert model_plan(curve, group, n, config, {}, lgk=6)[6] == 1
    run_both_sets(variant_ctx, inputs, capfd, monkeypatch, config, {}, lgk=6)


# ------------------------------------------------------------------------------------------- E: sort
SORT = ([({}, {"ZKP_SORT_STAGED": 0})] + [({}, {"ZKP_SORT_H1": h}) for h in (1, 4, 11, 12, 13)] +
        [(bits(22), {"ZKP_SORT_H1": 13}), (bits(22), {"ZKP_SORT_H1": 4})] +
        [({}, {"ZKP_SORT_NT_HIST": h, "ZKP_SORT_NT_SCATTER": s}) for h, s in ((256, 256), (512, 1024), (1024, 256))] +
        [({}, {"ZKP_TASK_NT": t}) for t in (256, 512)])


@pytest.mark.parametrize("config,env", SORT, ids=ids(SORT))
def test_sort_variants(variant_ctx, inputs, capfd, monkeypatch, config, env):
    """E: the unstaged level-1 scatter; forced level-1 bits (12, 13: more than 2048 bins, where the staged scatter switches itself
    off; 4 with 22 window bits: 21 - 4 low bits exceed the level-2 limit of 13 and H1 is corrected to 8); every workgroup size of
    the level-1 passes and of the task kernels."""
    run_both_sets(variant_ctx, inputs, capfd, monkeypatch, config, env)


# ------------------------------------------------------------------------------------------- F: tasks
TASKS = ([({}, {"ZKP_TASK_CAP": t}) for t in (4, 5, 127, 128)] + [({}, {"ZKP_TASK_CAP": 128, "ZKP_TASK_CAP_G2": 4})] +
         [({}, {"ZKP_MEMSET_BUCKETS": 1}), ({}, {"ZKP_DEBUG_FORCE_REDO": 1}), ({}, {"ZKP_DEBUG_FORCE_REDO": 1, "ZKP_TASK_CAP": 4})])


@pytest.mark.parametrize("config,env", TASKS, ids=ids(TASKS))
def test_task_variants(variant_ctx, inputs, capfd, monkeypatch, config, env):
    """F: entries per task (4: the 301 equal scalars make 76 tasks per bucket — the wave-per-bucket combine), the whole-array
    memset, every eighth task through the exact redo kernel."""
    run_both_sets(variant_ctx, inputs, capfd, monkeypatch, config, env)


# ------------------------------------------------------------------------------------------- G: reduction
REDUCE = [(bits(c), env) for env in ([{"ZKP_PAIR_TOP": 0}, {"ZKP_PAIR_TOP_FUSE_SEG": 0}] + [{"ZKP_PAIR_TOP_MAX": m} for m in (2, 4, 512, 4096)])
          for c in (2, 10, 13, 14)]


@pytest.mark.parametrize("config,env", REDUCE, ids=ids(REDUCE))
def test_reduction_variants(variant_ctx, inputs, capfd, monkeypatch, config, env):
    """G: the pyramid by plain pair launches, the top as a launch of its own, and the top cut at 2, 4, 512 and 4096 entries with
    2, 512, 4096 and 8192 buckets: below, at and above every cut."""
    run_both_sets(variant_ctx, inputs, capfd, monkeypatch, config, env)


@pytest.mark.parametrize("env", [{"ZKP_PAIR_TOP": 0}, {"ZKP_PAIR_TOP_MAX": 4}], ids=["PAIR_TOP=0", "PAIR_TOP_MAX=4"])
def test_reduction_variants_exceptional_bucket_sums(variant_ctx, inputs, capfd, monkeypatch, env):
    """G: equal and opposite BUCKET sums meeting in the pyramid (tests/test_gpu_msm.py
    test_msm_reduction_pyramid_exceptional_cases) under the plain pair launches and under a top of four entries."""
    with variant_ctx(inputs("bn254", 1).ctx.device, {}, env) as v:
        for curve, group in CFG:
            I = inputs(curve, group)
            G = I.G
            Q, R = random_points(curve, group, 2, seed=77 + group)
            for pts, ks in [([Q, Q], [1, 2]), ([Q, G.neg(Q)], [1, 2]), ([Q, R, Q, R], [1, 2, 3, 4]),
                            ([Q, R, G.neg(Q), G.neg(R)], [1, 2, 3, 4]), ([Q] * 8, [1, 2, 3, 4, 5, 6, 7, 8])]:
                xy, inf = to_abi_points(curve, group, pts)
                with uploaded(v, capfd, monkeypatch, I, xy, inf, model_plan(curve, group, len(pts), {}, env)) as b:
                    assert affine(I, b.msm(codec.fr_canonical(ks, I.c).reshape(-1, 4))) == G.msm_naive(pts, ks), (curve, group, ks)


# ------------------------------------------------------------------------------------------- H: variable-base
@pytest.mark.parametrize("var_c", [4, 8, 16, None])
def test_variable_base_window_bits(variant_ctx, inputs, var_c):
    """H: zkp_msm_g*_var with 4 (64 bucket sets of 8 buckets, 64 windows: the unstaged scatter), 8 and 16 window bits and with the
    size rule (8 below 4096 points, 16 from there on), canonical and Montgomery scalars, flags absent / all clear / one set."""
    with variant_ctx(inputs("bn254", 1).ctx.device, {}, {} if var_c is None else {"ZKP_MSM_VAR_C": var_c}) as v:
        for curve, group in CFG:
            I = inputs(curve, group)
            c, lo = I.c, 8                                           # the slice starts behind the set's identity base
            for n in (0, 1, 24, 4095, 4096):
                ks = 988 if n <= 24 else 500                         # 24: 12 scalars, then equal ones; else the 301 equal ones inside
                xy, d, k = I.multi_xy[lo:lo + n], I.multi_d[lo:lo + n], I.multi_k[ks:ks + n]
                assert len(xy) == len(d) == len(k) == n              # a short slice would quietly run a smaller MSM
                can, mont = codec.fr_canonical(k, c).reshape(-1, 4), codec.fr_to_mont(k, c).reshape(-1, 4)
                want = I.point(sum(a * b for a, b in zip(d, k)))
                clear = np.zeros(n, dtype=np.uint8)
                for inf in (None, clear):
                    assert affine(I, v.msm_var(c, group, xy, inf, can)) == want, (curve, group, n)
                    assert affine(I, v.msm_var(c, group, xy, inf, mont, montgomery=True)) == want, (curve, group, n)
                if n > 1:
                    one = clear.copy()
                    one[n // 2] = 1
                    want = I.point(sum(a * b for i, (a, b) in enumerate(zip(d, k)) if i != n // 2))
                    assert affine(I, v.msm_var(c, group, xy, one, can)) == want, (curve, group, n)
                    assert affine(I, v.msm_var(c, group, xy, one, mont, montgomery=True)) == want, (curve, group, n)


# ------------------------------------------------------------------------------------------- I: accumulate instantiations
ACC = [({}, {"ZKP_G1_ACC_OCC": 4}), ({}, {"ZKP_G1_ACC_WAVES": 3}), ({}, {"ZKP_G2_ACC_OCC": 1}), ({}, {"ZKP_G2_ACC_OCC": 3}),
       ({}, {"ZKP_ACC_LDS_BYTES": 16384})]


@pytest.mark.parametrize("config,env", ACC, ids=ids(ACC))
def test_accumulate_instantiations(variant_ctx, inputs, capfd, monkeypatch, config, env):
    """I: every compiled instantiation of the accumulate kernel on both sets, and an input whose buckets run into the fast path's
    exceptional cases WITHOUT the debug switch: five bases with ONE scalar land in one bucket of every window; A, B with A + B = P
    followed by P (a doubling) or by -P (a cancellation) and two ordinary bases behind them, plus P, P, X and P, -P, X.  (The order
    inside a bucket is the sort's; whichever it is, the sum is the same, and every abandoned task goes through the redo kernel.)"""
    with variant_ctx(inputs("bn254", 1).ctx.device, config, env) as v:
        for curve, group in CFG:
            I = inputs(curve, group)
            check_edge(v, capfd, monkeypatch, I, config, env)
            check_multi(v, capfd, monkeypatch, I, config, env)
            r = I.c.r
            rnd = random.Random(31 * group)
            a, p, x, y, a2, p2, x2, y2, p3, x3, p4, x4 = [rnd.randrange(1, r) for _ in range(12)]
            d = [a, (p - a) % r, p, x, y, a2, (p2 - a2) % r, r - p2, x2, y2, p3, p3, x3, p4, r - p4, x4]
            s = [rnd.randrange(r) for _ in range(4)]
            k = [s[0]] * 5 + [s[1]] * 5 + [s[2]] * 3 + [s[3]] * 3
            xy, inf = I.ctx.fixed_base_mul(I.c, group, I.g_xy, codec.fr_canonical(d, I.c))
            with uploaded(v, capfd, monkeypatch, I, xy, inf, model_plan(curve, group, len(d), config, env)) as b:
                assert affine(I, b.msm(codec.fr_canonical(k, I.c).reshape(-1, 4))) == I.dot(d, k, len(d), 0), (curve, group)


# ------------------------------------------------------------------------------------------- J: chunking
CHUNKS = [(dict(msm_chunk_points=1024), {"ZKP_MSM_CHUNK_FIRST": f}) for f in (1, 2, 3)] + [(dict(msm_chunk_points=1500), {})]


@pytest.mark.parametrize("config,env", CHUNKS, ids=ids(CHUNKS))
def test_chunked_msm_at_the_smallest_chunk(variant_ctx, inputs, capfd, monkeypatch, config, env):
    """J (G1): the public minimum of 1024 points per chunk with n just below, at and above 2 * 1024 — per rounded to 256, a first
    chunk of at least 1024 points, a ragged last one — and 1500 (no multiple of 256) at the multi-tile size.  Three calls in a row
    (the workspaces are reused) equal the oracle and the session context's unchunked result; one batch call keeps two chunked
    MSMs in flight.  The library reports no chunk lengths: the split of tests/msm_plan_ref.py only says which sizes are chunked at
    all and labels a failure; what is verified here is the result."""
    cp, first = config["msm_chunk_points"], env.get("ZKP_MSM_CHUNK_FIRST", 2)
    sizes = (2047, 2048, 2049, 2304, N_MULTI) if cp == 1024 else (N_MULTI,)
    assert [len(M.chunk_lengths(n, cp, first)) > 1 for n in sizes] == [n >= 2 * cp for n in sizes]
    with variant_ctx(inputs("bn254", 1).ctx.device, config, env) as v:
        assert v.config()["msm_chunk_points"] == cp
        for curve, group in G1:
            I = inputs(curve, group)
            with uploaded(v, capfd, monkeypatch, I, I.multi_xy, I.multi_inf, model_plan(curve, group, N_MULTI, config, env)) as b:
                for n in sizes:
                    for _ in range(3):
                        got = affine(I, b.msm(I.multi[:n]))
                        assert got == I.multi_exp(n, 0) and got == I.multi_default(n, 0), (curve, n, M.chunk_lengths(n, cp, first))
                kd = v.to_device(I.multi_mont())
                try:
                    outs = b.msm_mont_batch_dev([(kd, N_MULTI, 0), (kd + 32 * 10, N_MULTI - 10, 10)])
                finally:
                    v.dev_free(kd)
                assert affine(I, outs[0]) == I.multi_exp(N_MULTI, 0)
                assert affine(I, outs[1]) == I.point(sum(a * b for a, b in zip(I.multi_d[10:], I.multi_k[10:])))


# ------------------------------------------------------------------------------------------- K: nothing is left for the next MSM
def test_no_chain_request_outlives_its_msm(ctx, inputs):
    """One context, in this order: a stand-alone MSM; a Groth16 proof at 2^6 whose L query defers its reduction to H (the bucket
    chain travels in each MSM's own request); the stand-alone MSM refused for a freed bases handle; the stand-alone MSM again,
    with the first call's result."""
    from tests.test_gpu_groth16_fused import _setup
    I = inputs("bn254", 1)
    b = ctx.upload_bases(I.c, 1, I.multi_xy, I.multi_inf)
    gone = ctx.upload_bases(I.c, 1, I.multi_xy[:N_EDGE], I.multi_inf[:N_EDGE])
    pk, c, zs = _setup(ctx, "bn254", 6)
    try:
        first = b.msm(I.multi)
        assert affine(I, first) == I.multi_exp(N_MULTI, 0)
        assert pk.table_plan()["l_h_bucket_chained"]
        one = codec.fr_to_mont([1], c).reshape(-1, 4)
        out, _ = pk.prove_raw(zs[0], one[0], one[0], z_on_device=False)
        assert out.any()
        stale = gone.handle
        gone.free()
        gone.handle = stale
        with pytest.raises(_lib.ZkpError) as err:
            gone.msm(I.multi[:N_EDGE])
        assert err.value.status == -6                                          # include/zkp_accel.h ZKP_ERR_BAD_HANDLE
        assert affine(I, b.msm(I.multi)) == affine(I, first)                   # (the Jacobian limbs depend on the order inside a bucket)
    finally:
        gone.handle = 0
        pk.free()
        b.free()
