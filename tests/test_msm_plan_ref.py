"""CPU: invariants of the window-plan model (tests/msm_plan_ref.py) that tests/test_gpu_msm_plans.py holds the device against.

For every window size 2 .. 22, both scalar widths, balanced and equal windows and every window-group size: the widths cover the
scalar, the signed digits of edge and random scalars recombine to the scalar with no carry left and stay inside the bucket range;
the default rule is pinned at the sizes where it changes; the chunk split covers n in multiples of 256."""
import math
import random

import pytest

from oracle.pyref import fields as ofields
from tests import msm_plan_ref as M

R = {"bn254": ofields.BN254.r, "bls12_381": ofields.BLS12_381.r}


def test_the_switch_table_is_read_whole():
    """tests/test_gpu_msm_plans.py clears these names before it creates a variant context: a reformatted table must not empty the list"""
    from tests.test_tune_table import DEFAULTS
    names = M.tune_switch_names()
    assert len(names) == len(set(names)) and set(names) == set(DEFAULTS)


def test_scalar_widths_match_the_group_orders():
    assert {k: v.bit_length() for k, v in R.items()} == M.SCALAR_BITS


def edge_scalars(r, c, W, wide, scalar_bits, rnd):
    ones = (1 << (r.bit_length() - 1)) - 1                                   # all-ones below r
    return [0, 1, r - 1, r - 2, (r - 1) // 2, ones, *M.threshold_scalars(c, W, wide, scalar_bits)] + [rnd.randrange(r) for _ in range(200)]


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
@pytest.mark.parametrize("balanced", [True, False])
@pytest.mark.parametrize("c0", range(2, 23))
def test_windows_cover_the_scalar_and_digits_recombine(curve, balanced, c0):
    r, bits = R[curve], M.SCALAR_BITS[curve]
    T = bits + 1
    rnd = random.Random(c0 * 4 + balanced)
    for lgk in range(7):
        c, W, wide, lgk_out, J = M.window_plan(bits, 1000, 1, c0, lgk, balanced)
        widths = M.window_widths(c, W, wide)
        assert len(widths) == W and 1 <= wide <= W and min(widths) >= 1
        if balanced and lgk == 0:
            assert sum(widths) == T and c <= c0 and max(widths) - min(widths) <= 1
        else:
            assert T <= sum(widths) < T + c and wide == W                 # equal widths: only the top window reaches past T
        assert M.window_positions(c, W, wide)[-1] == sum(widths)
        if lgk == 0:
            assert (lgk_out, J) == (0, W)
        else:
            assert c == max(4, c0 - lgk) and J == -(-W // (1 << lgk_out)) and (J - 1) << lgk_out < W
            assert lgk_out == lgk or (J == 1 and 1 << lgk_out >= W > 1 << (lgk_out - 1))
        for k in edge_scalars(r, c, W, wide, bits, rnd):
            assert 0 <= k < r
            digits, carry = M.signed_digits(k, c, W, wide)
            assert carry == 0, (k, c, W, wide)
            assert M.recombine(digits, c, W, wide) == k
            assert all(abs(d) <= 1 << (cw - 1) for d, cw in zip(digits, widths))


@pytest.mark.parametrize("curve", ["bn254", "bls12_381"])
def test_threshold_scalars_sit_on_both_sides_of_the_sign_change(curve):
    bits = M.SCALAR_BITS[curve]
    for c0 in range(2, 23):
        c, W, wide, _, _ = M.window_plan(bits, 0, 1, c0, 0, True)
        at, above = M.threshold_scalars(c, W, wide, bits)
        widths, pos = M.window_widths(c, W, wide), M.window_positions(c, W, wide)
        full = [w for w in range(W) if pos[w] + widths[w] <= bits - 1]
        d_at, d_above = M.signed_digits(at, c, W, wide)[0], M.signed_digits(above, c, W, wide)[0]
        assert full and all(d_at[w] == 1 << (widths[w] - 1) for w in full)          # the largest positive digit, no carry
        # one more: 2^(cw-1) + 1 - 2^cw, plus the carry of the window below, and a carry into the window above
        assert all(d_above[w] == 1 - (1 << (widths[w] - 1)) + (w > 0) for w in full)
        assert d_above[full[-1] + 1] == 1


def test_default_rule_is_pinned_where_it_changes():
    pick = M.pick_window_bits
    # clamp at 4; rounding at sqrt(2) 2^k (724 < 724.08 < 725, 1448 < 1448.15 < 1449); + 3 from round(log2 n) = 10 on
    want = {0: 4, 1: 4, 16: 4, 22: 4, 23: 5, 724: 9, 725: 13, 1023: 13, 1024: 13, 1448: 13, 1449: 14, 4609: 15, 23170: 17, 23171: 17,
            (1 << 15) - 1: 17, 46340: 17, 46341: 18, (1 << 17): 19, 185364: 19, 185365: 19, (1 << 19): 20, (1 << 20): 20, (1 << 24): 20}
    assert {n: pick(n, 1, True) for n in want} == want
    plain = {16: 4, 724: 9, 725: 10, 1449: 11, 4609: 12, (1 << 17): 17, (1 << 19): 19, (1 << 22): 20}
    assert {n: pick(n, 1, True, widen=False) for n in plain} == plain
    assert {n: pick(n, 2, False) for n in plain} == plain                            # a key's query: never widened
    # configured bits: G2 bases take msm_c_g2 first, anything outside 2 .. 22 is "not set"
    assert pick(5000, 1, True, msm_c=7) == 7 and pick(5000, 2, True, msm_c=7) == 7
    assert pick(5000, 2, True, msm_c=7, msm_c_g2=22) == 22 and pick(5000, 1, True, msm_c=7, msm_c_g2=22) == 7
    assert pick(5000, 1, True, msm_c=23) == 15 and pick(5000, 2, True, msm_c_g2=1) == 15
    for k in range(2, 40):
        assert M.round_log2(1 << k) == k and M.round_log2((1 << k) - 1) == k and M.round_log2((1 << k) + 1) == k
    # the library's decimal 1.41421356 for sqrt(2): the smallest n it rounds differently is beyond what an upload accepts
    differ = [n for k in range(40) for n in range(-(-141421356 * 2 ** k // 10 ** 8), math.isqrt(2 * 4 ** k) + 1)][:1]
    assert differ == [189812531] and M.round_log2(differ[0]) == 27 and M.round_log2(differ[0] + 1) == 28
    assert differ[0] > (1 << 31) // -(-255 // 20) == 165191049


def test_plans_named_in_the_design():
    # c = 20 on a 254-bit field: 8 windows of 20 and 5 of 19 bits (msm.hip); equal widths: 13 of 20
    assert M.window_plan(254, 1 << 20, 1, 0, 0, True) == (20, 13, 8, 0, 13)
    assert M.window_plan(254, 1 << 20, 1, 0, 0, False) == (20, 13, 13, 0, 13)
    # c = 2: 128 windows; 255 bits leave the top one a single bit wide, 256 bits fill it
    assert M.window_plan(254, 48, 1, 2, 0, True) == (2, 128, 127, 0, 128)
    assert M.window_plan(255, 48, 1, 2, 0, True) == (2, 128, 128, 0, 128)
    # 21 bits asked, 13 windows needed: balanced windows are 20 and 19 bits wide
    assert M.window_plan(254, 48, 1, 21, 0, True) == (20, 13, 8, 0, 13)
    # window groups: 2^20 points, tables 13 / 7 / 4 / 2 / 1 copies (msm.hip bases_upload)
    assert [M.window_plan(254, 1 << 20, 1, 0, lgk, True)[4] for lgk in range(5)] == [13, 7, 4, 2, 1]
    assert M.window_plan(254, 48, 1, 5, 2, True) == (4, 64, 64, 2, 16)               # max(4, 5 - 2)
    assert M.window_plan(254, 48, 1, 5, 6, True) == (4, 64, 64, 6, 1)
    assert M.window_plan(254, 4609, 1, 0, 6, True) == (9, 29, 29, 5, 1)              # k >= W: k = the next power of two >= W
    assert [M.table_lgk(k) for k in (0, 1, 2, 3, 4, 16, 64, 100)] == [0, 0, 1, 2, 2, 4, 6, 6]


@pytest.mark.parametrize("chunk_first", [1, 2, 3, 7])
def test_chunks_cover_n_in_multiples_of_256(chunk_first):
    rnd = random.Random(chunk_first)
    sizes = {2047, 2048, 2049, 2303, 2304, 2305, 3071, 3072, 3073, 4096, 4609, 1 << 18, (1 << 18) + 777, 300001}
    for cp in (1024, 1025, 1279, 1280, 1500, 2048, 40000, 1 << 16, 100000):
        for n in sorted(sizes | {2 * cp - 1, 2 * cp, 2 * cp + 1, 3 * cp, 3 * cp + 1} | {rnd.randrange(1, 40 * cp) for _ in range(300)}):
            ch = M.chunk_lengths(n, cp, chunk_first)
            assert sum(ch) == n and all(x > 0 for x in ch), (n, cp, ch)
            assert all(x % 256 == 0 for x in ch[:-1]), (n, cp, ch)
            assert len(ch) >= 2 if n >= 2 * cp else ch == [n], (n, cp, ch)
            assert len(ch) == 1 or max(ch) <= cp + 255, (n, cp, ch)                   # no chunk grows past what was asked (+ rounding)
    assert M.chunk_lengths(5000, 0) == [5000] and M.chunk_lengths(5000, 1000) == [5000]
    assert M.chunk_lengths(2049, 1024, 2) == [1024, 768, 257] and M.chunk_lengths(2049, 1024, 1) == [768, 768, 513]
    assert M.chunk_lengths(4609, 1500, 2) == [1024, 1280, 1280, 1025]
