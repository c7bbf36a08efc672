"""A plain-integer model of the MSM window plan, written from the prose of DESIGN.md and of the comments in csrc/msm.hip and
csrc/msm_digits.hpp.

Nothing here is taken from the device or from the library: tests/test_msm_plan_ref.py checks the model's own invariants on the
CPU, tests/test_gpu_msm_plans.py compares the plan the library prints at upload with this one and builds its edge scalars from it.
sort_plan / sched_layout model the geometry of the bucket sort and of the task schedule; tests/test_msm_sort_plan.py compares
csrc/msm_sort_plan.hpp with them.

One place where the model is exact and the library is not: round(log2 n) turns at sqrt(2) 2^k, which the library writes as the
decimal 1.41421356.  The two disagree only for an integer n in [1.41421356 2^k, sqrt(2) 2^k); the smallest such n is 189812531
(k = 27), and the rule never sees it: it yields at most 20 bits, hence at least 13 windows, and an upload requires n W < 2^31, that
is n < 165191050 (tests/test_msm_plan_ref.py pins both numbers).

    T = scalar_bits + 1          one spare bit absorbs the last signed-digit carry
    c                            bucket bits: a window's digits lie in [-2^(c-1), 2^(c-1)], 2^(c-1) buckets
    W                            windows; the first `wide` are c bits wide, the other W - wide are c - 1 (balanced windows)
    k = 2^lgk                    window-group size: k consecutive windows share one table copy and use k bucket sets
    J = ceil(W / k)              resident table copies
"""

import re
from pathlib import Path

SCALAR_BITS = {"bn254": 254, "bls12_381": 255}
C_MIN, C_MAX = 2, 22                     # zkp_ctx_config.msm_window_bits / msm_window_bits_g2


def round_log2(n: int) -> int:
    """round(log2 n) with the half-way point at sqrt(2) * 2^k, in exact integer arithmetic; 0 for n < 2."""
    lg = max(n, 1).bit_length() - 1
    return lg + 1 if n * n >= 1 << (2 * lg + 1) else lg


def pick_window_bits(n: int, group: int, lone: bool, msm_c: int = 0, msm_c_g2: int = 0, widen: bool = True) -> int:
    """Window bits of a base vector of n points.  A configured value (G2 bases: msm_c_g2 first) wins.  Otherwise round(log2 n); a
    LONE base vector (uploaded on its own, not a query of a Groth16 key) of 2^10 points or more takes wider windows unless `widen`
    is off: + 3 up to 2^14, + 2 up to 2^17, + 1 up to 2^19, + 0 from 2^20; the result is clamped to 4 .. 20."""
    if group == 2 and C_MIN <= msm_c_g2 <= C_MAX:
        return msm_c_g2
    if C_MIN <= msm_c <= C_MAX:
        return msm_c
    lg = round_log2(n)
    if lone and widen and lg >= 10:
        lg += 3 if lg <= 14 else 2 if lg <= 17 else 1 if lg <= 19 else 0
    return min(20, max(4, lg))


def window_plan(scalar_bits: int, n: int, group: int, c_hint: int, lgk: int, balanced: bool, lone: bool = True, msm_c: int = 0,
                msm_c_g2: int = 0, widen: bool = True):
    """-> (c, W, wide, lgk, J).  c_hint in 2 .. 22: the caller's window bits; anything else: pick_window_bits.

    lgk == 0: W = ceil(T / c0) windows.  Balanced: T is spread over them as ceil(T / W) and floor(T / W) bits, `wide` of the
    former; not balanced: W windows of c0 bits (the top one reaches past bit T).
    lgk > 0 (window groups): c = max(4, c0 - lgk) keeps the bucket count of the k bucket sets together near 2^(c0 - 1), equal
    widths; a group size of W or more is one table copy, and k becomes the next power of two >= W."""
    T = scalar_bits + 1
    c0 = c_hint if C_MIN <= c_hint <= C_MAX else pick_window_bits(n, group, lone, msm_c, msm_c_g2, widen)
    if lgk <= 0:
        W = -(-T // c0)
        if not balanced:
            return c0, W, W, 0, W
        c = -(-T // W)
        return c, W, T - W * (c - 1), 0, W
    c = max(4, c0 - lgk)
    W = -(-T // c)
    if (1 << lgk) >= W:
        lgk = (W - 1).bit_length()
    return c, W, W, lgk, -(-W // (1 << lgk))


def window_widths(c: int, W: int, wide: int):
    return [c if w < wide else c - 1 for w in range(W)]


def window_positions(c: int, W: int, wide: int):
    """bit position of every window, and of the end of the last one"""
    pos, out = 0, []
    for cw in window_widths(c, W, wide):
        out.append(pos)
        pos += cw
    return out + [pos]


def signed_digits(k: int, c: int, W: int, wide: int):
    """-> (digits, last carry).  Window w holds the cw bits of k at its position plus the carry of the window below; a value ABOVE
    2^(cw-1) becomes value - 2^cw and carries one into the next window (2^(cw-1) itself stays positive: the bucket range is
    1 .. 2^(cw-1))."""
    digits, carry, pos = [], 0, 0
    for cw in window_widths(c, W, wide):
        d = ((k >> pos) & ((1 << cw) - 1)) + carry
        carry = 0
        if d > 1 << (cw - 1):
            d -= 1 << cw
            carry = 1
        digits.append(d)
        pos += cw
    return digits, carry


def recombine(digits, c: int, W: int, wide: int) -> int:
    return sum(d << p for d, p in zip(digits, window_positions(c, W, wide)))


def threshold_scalars(c: int, W: int, wide: int, scalar_bits: int):
    """Two scalars below 2^(scalar_bits - 1) (hence below r): every window that lies wholly below that bit holds the raw digit
    2^(cw-1) (the largest that stays positive) / 2^(cw-1) + 1 (the smallest that turns negative and carries; a one-bit window
    cannot hold it and keeps 1)."""
    at = above = 0
    for cw, pos in zip(window_widths(c, W, wide), window_positions(c, W, wide)):
        if pos + cw <= scalar_bits - 1:
            at |= (1 << (cw - 1)) << pos
            above |= min((1 << (cw - 1)) + 1, (1 << cw) - 1) << pos
    return at, above


def table_lgk(table_k: int) -> int:
    """ZKP_TABLE_K: the forced group size, rounded up to a power of two, at most 64"""
    return (min(max(table_k, 1), 64) - 1).bit_length()


def chunk_lengths(n: int, chunk_points: int, chunk_first: int = 2):
    """Chunk lengths of a stand-alone G1 MSM of n points (msm.hip msm_run).  Chunked from 2 * chunk_points on (chunk_points >= 1024).
    ceil(n / chunk_points) chunks of `per` points, per a multiple of 256; with chunk_first > 1 the first chunk is per / chunk_first
    points (a multiple of 256, at least 1024) and the rest is split evenly, again in multiples of 256; the last chunk takes what is
    left."""
    if chunk_points < 1024 or n < 2 * chunk_points:
        return [n]
    up = lambda x: (x + 255) & ~255
    per = up(-(-n // -(-n // chunk_points)))
    out = []
    rest = n
    if chunk_first > 1:
        first = max(up(per // chunk_first), 1024)
        if first < n:
            out.append(first)
            rest = n - first
    per_rest = up(-(-rest // -(-rest // per)))
    while rest > 0:
        out.append(min(per_rest, rest))
        rest -= out[-1]
    return out


# The bucket sort and the task schedule (csrc/msm.hip K6 / K7), as the host code sized them before csrc/msm_sort_plan.hpp existed
SORT_H1_MAX, SORT_L_MAX = 13, 13         # level-1 bins <= 8192 (static LDS histogram), level-2 keys per bin <= 8192
SORT_BIN_TARGET = 16384                  # entries per level-1 bin the level-2 kernel stages in LDS
SORT_SCALARS = 2048                      # scalars per level-1 tile, more for large MSMs
SORT_STAGE_BYTES = 56 * 1024             # LDS stage of the staged level-1 scatter
SORT_BIN_STAGE = 20480                   # values the level-2 kernel stages in LDS
TM_WORDS = 512                           # the schedule's tmeta block
U32 = 0xFFFFFFFF


def sort_plan(n: int, W: int, sets: int, kbits: int, forced_h1: int = 0, staged_enabled: bool = True):
    """-> None when the shape is refused, else a dict.  E = n W sets entries go into 2^H1 level-1 bins: 10 bits, more (up to 13)
    while a bin would hold more than SORT_BIN_TARGET entries; a forced value (> 0, at most 13) replaces that; never more than
    the kbits of a bucket id, and at least kbits - 13 so that a bin has at most 2^13 keys.  Refused when H1 < log2(sets): a bin
    would straddle two scalar vectors.  Tiles of 2048 scalars, grown by 256 until there are at most 1536 of them.  The staged
    scatter runs with at most 2048 bins per vector when 256 scalars' entries (8 bytes each) fit the stage, in sub-rounds of as
    many scalars as fit, a multiple of 256, at most a tile."""
    lgs = (sets - 1).bit_length()
    E = n * W * sets
    H1 = 10
    while H1 < SORT_H1_MAX and (E >> H1) > SORT_BIN_TARGET:
        H1 += 1
    if forced_h1 > 0:
        H1 = min(SORT_H1_MAX, forced_h1)
    H1 = min(H1, kbits)
    if kbits - H1 > SORT_L_MAX:
        H1 = kbits - SORT_L_MAX
    if H1 < lgs:
        return None
    LB = kbits - H1
    nbins1 = 1 << H1
    nbins_set = nbins1 >> lgs
    tile = SORT_SCALARS
    while -(-n // tile) > 1536:
        tile += 256
    nblocks = -(-n // tile)
    staged_sub = staged_lds = 0
    if staged_enabled and nbins_set <= 2048 and 256 * W * 8 <= SORT_STAGE_BYTES:
        staged_sub = min(SORT_STAGE_BYTES // (W * 8) // 256 * 256, tile)
        staged_lds = (nbins_set + ((nbins_set + 3) & ~3)) * 4 + staged_sub * W * 8
    return dict(H1=H1, LB=LB, nbins1=nbins1, nbins_set=nbins_set, tile=tile, nblocks=nblocks, hist_n=nbins1 * nblocks + 1,
                staged_sub=staged_sub, staged_lds=staged_lds, bin_lds=(4 << LB) + 4 * SORT_BIN_STAGE)


def sched_layout(nb: int, E: int, cap: int):
    """The schedule's arrays in one buffer of 32-bit words: tcount and toff (nb + 2 words each), task_start, task_len, task_dst and
    long_list (max_tasks each), tmeta (TM_WORDS), then, at the next 16-byte boundary, max_tasks 16-byte descriptors; 8 words spare.
    max_tasks = nb + E / cap + 1 in 32-bit arithmetic."""
    max_tasks = (nb + ((E // cap) & U32) + 1) & U32
    out = dict(max_tasks=max_tasks, words=2 * (nb + 2) + 8 * max_tasks + TM_WORDS + 8, tcount=0, toff=nb + 2)
    at = 2 * (nb + 2)
    for name in ("task_start", "task_len", "task_dst", "long_list", "tmeta"):
        out[name] = at
        at += max_tasks
    out["desc_bytes"] = ((out["tmeta"] + TM_WORDS) * 4 + 15) & ~15
    return out


def tune_switch_names():
    """the environment names of the internal switches, in the order of the table in csrc/tune.hpp (ZKP_TUNE_ROWS)"""
    text = (Path(__file__).resolve().parent.parent / "ckb_zkp_amd" / "csrc" / "tune.hpp").read_text()
    return re.findall(r'^\s*(?:FLAG|INT|MASK)\s*\(\s*\w+\s*,\s*"(ZKP_\w+)"', text, flags=re.M)
