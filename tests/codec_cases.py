"""Edge inputs for the point codec and the subgroup check (zkp_g1/g2_decompress, _compress, _subgroup_check: the "point codec"
section of csrc/msm_group.hip), built from the curves' own constants (oracle.pyref.fields through tests.util.OC and
oracle.pyref.curves.Group) and judged by the oracle codec (oracle/pyref/serialize.py).  Pure Python, no GPU import: the lists are
pinned on the CPU by tests/test_codec_cases.py and run on the device by tests/test_gpu_codec_edges.py.

No coordinate is written down here: small integers only start searches.  Every list is deterministic and every case has a name.

  (a) decompress_cases   byte strings; the verdict is `oser.point_decode(..., checked=False)`: a point, None, or INVALID
  (b) compress_cases     affine coordinates as integers, NOT necessarily on the curve.  Neither `compress_kernel` nor
                         `oser.point_encode` tests the curve equation, so an off-curve y exercises the sign logic alone.
  (c) subgroup_cases     Montgomery integers per coordinate (so that "off by one in the lowest Montgomery word" can be said);
                         the verdict is `G.on_curve` and `oser.in_subgroup` of the canonical point they stand for
  (d) failure_layouts    sizes and bad-index sets for the 64-lane grid

What stays unreached: no G1 point of either curve has y = (p - 1) / 2 (y^2 - b is not a cubic residue on either, see
`no_g1_point_at_half_p`), and an on-curve y within 2^(32 k) of p / 2 would need a cube-root search per limb.  The lower limbs of
`fp_gt` are therefore reached through compress (b) only, never through decompress.
"""
from collections import Counter, namedtuple
from functools import lru_cache
import random

from oracle.pyref import serialize as oser
from oracle.pyref.curves import Group
from tests.util import OC

CURVES = ("bn254", "bls12_381")
PAIRS = [(curve, group) for curve in CURVES for group in (1, 2)]
INVALID = "InvalidData"                                # the third verdict of (a), beside a point and None
POS, INF = oser.POSITIVE_Y, oser.INFINITY
POOL = 200

DecCase = namedtuple("DecCase", "name kind data want")            # want: (x, y) | None | INVALID
CompCase = namedtuple("CompCase", "name kind x y inf want")       # inf: 0 | 1 | None (no inf array at all); want: bytes
SubCase = namedtuple("SubCase", "name kind mont inf want")        # mont: 2 (G1) or 4 (G2) Montgomery integers; want: bool
Layout = namedtuple("Layout", "n bad first")


def limbs32(curve):
    """32-bit limbs of the base field in the kernels (P::N)"""
    return 2 * OC[curve].fq_limbs


def _uniq(seq):
    return list(dict.fromkeys(seq))


def field_edges(curve):
    """canonical values at the ends of the field and on every 32-bit limb boundary"""
    p = OC[curve].q
    v = [0, 1, 2, 3, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1]
    for k in range(limbs32(curve)):
        v += [1 << (32 * k), (1 << (32 * k)) - 1]
    assert all(0 <= e < p for e in v)
    return _uniq(v)


def y_edges(curve):
    """y values whose order against -y is decided at the ends of the field and, for (p -+ 1) / 2 -+ 2^(32 k), at limb k: there
    y and -y = p - y agree in every limb above k.  Closed under negation."""
    p = OC[curve].q
    v = [1, 2, p - 2, p - 1, (p - 1) // 2, (p + 1) // 2]
    for k in range(limbs32(curve)):
        for e in ((p - 1) // 2 - (1 << (32 * k)), (p + 1) // 2 + (1 << (32 * k))):
            if 1 <= e <= p - 1:
                v.append(e)
    v = _uniq(v)
    assert all((p - e) in v for e in v)
    return v


def encode_raw(curve, group, vals, flags=0):
    """the integers `vals` (one for G1, c0 and c1 for G2) as ark lays them out, canonical or not, with `flags` on the last byte"""
    n = oser.fq_size(OC[curve])
    assert len(vals) == group
    out = bytearray(b"".join(int(v).to_bytes(n, "little") for v in vals))
    out[-1] |= flags
    return bytes(out)


def verdict(curve, group, data):
    try:
        return oser.point_decode(data, OC[curve], group, checked=False)
    except oser.InvalidData:
        return INVALID


@lru_cache(maxsize=None)
def pool(curve, group):
    """POOL distinct points of the prime-order subgroup: (k0 + i d) G, walked by affine additions (one scalar multiplication each
    for the start and the step, where POOL multiplications in Python integers would dominate the files that use this)"""
    G = Group(OC[curve], group)
    rnd = random.Random(f"codec pool {curve} {group}")
    P, D = G.mul(G.gen, rnd.randrange(1, G.order)), G.mul(G.gen, rnd.randrange(1, G.order))
    out = []
    for _ in range(POOL):
        out.append(P)
        P = G.add(P, D)
    assert len(set(out)) == POOL and None not in out and all(G.on_curve(Q) for Q in out[:3] + out[-3:])
    return tuple(out)


def _rand_fq(curve, tag):
    return random.Random(f"codec {curve} {tag}").randrange(2, OC[curve].q - 2)


# --------------------------------------------------------------------------------------------------------- (a) decompress
def zero_imaginary_xs(curve, need=4):
    """G2 x = (+-c0, c1) with Im(x^3 + b) = 0, i.e. c0^2 = (c1^3 - Im b) / (3 c1), for c1 = 1, 2, 3, ... until `need` values of c1
    gave an x whose y is real (Re(x^3 + b) a residue: y = (s, 0)) and `need` gave one whose y is imaginary (a non-residue:
    y = (0, s), since -1 is a non-residue).  The two signs of c0 give different real parts, so each x is classified on its own.
    -> [(c1, x, "real" | "imag", rhs)]"""
    oc = OC[curve]
    p, (b0, b1) = oc.q, oc.g2_b
    F = Group(oc, 2).F
    out, seen = [], {"real": set(), "imag": set()}
    c1 = 0
    while min(len(s) for s in seen.values()) < need:
        c1 += 1
        assert c1 < 400, "no Fq2 x with a zero imaginary part found"
        c0 = oser.sqrt_fp((c1 ** 3 - b1) * pow(3 * c1, -1, p), p)
        if c0 is None or c0 == 0:
            continue
        for s in (c0, p - c0):
            x = (s, c1)
            rhs = F.add(F.mul(F.sqr(x), x), (b0, b1))
            assert rhs[1] == 0, (curve, x)
            if rhs[0] == 0:
                continue
            kind = "real" if pow(rhs[0], (p - 1) // 2, p) == 1 else "imag"
            seen[kind].add(c1)
            out.append((c1, x, kind, rhs))
    return out


@lru_cache(maxsize=None)
def decompress_cases(curve, group):
    oc = OC[curve]
    p = oc.q
    n = oser.fq_size(oc)
    cases = []

    def add(name, kind, vals, flags):
        data = encode_raw(curve, group, vals, flags)
        cases.append(DecCase(f"{name} flags={flags:#04x}", kind, data, verdict(curve, group, data)))

    # canonical x: the oracle says which are on the curve
    edges = field_edges(curve)
    if group == 1:
        xs = [(f"x={e:#x}", (e,)) for e in edges]
    else:
        others = (("0", 0), ("1", 1), ("p-1", p - 1))
        xs = [(f"x=({e:#x}, {nm})", (e, o)) for e in edges for nm, o in others]
        xs += [(f"x=({nm}, {e:#x})", (o, e)) for e in edges for nm, o in others]
        xs = list(dict((v, (nm, v)) for nm, v in xs).values())                       # (0, 0), (1, 1), ... come up twice
    for name, vals in xs:
        for flags in (0, POS):
            add(name, "canonical", vals, flags)
    # G2: x^3 + b real, so that the square root leaves through `a.c1 == 0` and the sign through the c0 tie-break
    if group == 2:
        for c1, x, kind, rhs in zero_imaginary_xs(curve):
            for flags in (0, POS):
                add(f"Im(x^3+b)=0 c1={c1} c0={'+' if x[0] < p - x[0] else '-'} {kind} root", f"zero_im_{kind}", x, flags)
                y = cases[-1].want[1]
                assert cases[-1].want[0] == x and Group(oc, 2).F.sqr(y) == rhs
                assert (y[1] == 0 and y[0] != 0) if kind == "real" else (y[0] == 0 and y[1] != 0), (curve, x, y)
    # non-canonical coordinates: at and above the modulus, every bit below the flags, and on BLS12-381 the bits between the
    # modulus' top bit (380) and the flags (382, 383)
    top = 8 * n - 2
    bad = [("p", p), ("p+1", p + 1), (f"2^{top}-1", (1 << top) - 1)]
    if p.bit_length() < top:
        bad += [(f"2^{p.bit_length()}", 1 << p.bit_length())]
    assert all(p <= v < (1 << top) for _, v in bad) and len({v for _, v in bad}) == len(bad)
    gx = oc.g1_gen[0] if group == 1 else oc.g2_gen[0]
    for nm, v in bad:
        for flags in (0, POS, INF):
            if group == 1:
                add(f"x={nm}", "noncanonical", (v,), flags)
            else:
                add(f"x.c0={nm}, c1 valid", "noncanonical", (v, gx[1]), flags)
                add(f"x.c1={nm}, c0 valid", "noncanonical", (gx[0], v), flags)
    if group == 2:
        # c0 carries no flags: its top two bits are value bits (Fp::read of the whole 8 n bits)
        for flags in (0, POS, INF):
            add("x.c0 with bit 8n-1 set, c1 valid", "noncanonical", (gx[0] | (1 << (8 * n - 1)), gx[1]), flags)
    add("both flags on the generator's x", "both_flags", (gx,) if group == 1 else gx, POS | INF)
    add("both flags on x=0", "both_flags", (0,) * group, POS | INF)
    # the identity: canonical, and the flag beside a non-zero canonical x (ark reads x, then returns zero())
    add("identity", "identity", (0,) * group, INF)
    for v in (1, 5, p - 1):
        if group == 1:
            add(f"identity flag beside x={v:#x}", "identity", (v,), INF)
        else:
            add(f"identity flag beside x=({v:#x}, 0)", "identity", (v, 0), INF)
            add(f"identity flag beside x=(0, {v:#x})", "identity", (0, v), INF)
            add(f"identity flag beside x=({v:#x}, {v:#x})", "identity", (v, v), INF)
    for c in cases:
        if c.kind in ("noncanonical", "both_flags"):
            assert c.want == INVALID, c.name
        if c.kind == "identity":
            assert c.want is None, c.name
        if c.kind.startswith("zero_im"):
            assert c.want not in (None, INVALID), c.name
    return tuple(cases)


def no_g1_point_at_half_p(curve):
    """y = (p - 1) / 2 (and so y = (p + 1) / 2) is no G1 ordinate: y^2 - b is not a cube"""
    oc = OC[curve]
    p = oc.q
    assert p % 3 == 1
    t = (((p - 1) // 2) ** 2 - oc.g1_b) % p
    return pow(t, (p - 1) // 3, p) != 1


# ----------------------------------------------------------------------------------------------------------- (b) compress
@lru_cache(maxsize=None)
def compress_cases(curve, group):
    oc = OC[curve]
    p = oc.q
    ys = y_edges(curve)
    r0, r1, r2 = (_rand_fq(curve, t) for t in ("x", "c0", "x1"))
    cases = []

    def add(name, kind, x, y, inf=0, identity=False):
        want = oser.point_encode(None if identity else (x, y), oc, group)
        cases.append(CompCase(name, kind, x, y, inf, want))

    if group == 1:
        for y in ys:
            for nx, x in (("0", 0), ("1", 1), ("p-1", p - 1), ("random", r0)):
                add(f"y={y:#x} x={nx}", "y_edge", x, y)
        zero, junk = 0, r0
    else:
        xs = (("(0, 0)", (0, 0)), ("(1, p-1)", (1, p - 1)), ("random", (r0, r2)))
        for v in ys:
            for nx, x in xs:
                add(f"y=({v:#x}, 0) x={nx}", "y_tie", x, (v, 0))                    # decided by c0
                for nc, c0 in (("0", 0), ("1", 1), ("random", r1)):
                    add(f"y=({nc}, {v:#x}) x={nx}", "y_edge", x, (c0, v))          # decided by c1, whatever c0 is
        zero, junk = (0, 0), (r0, r2)
    # the identity: the flag wins over the words, (0, 0) words are the identity without a flag and without a flag array
    jy = ys[3] if group == 1 else (ys[3], ys[4])
    add("inf=1 beside non-zero words", "identity_rule", junk, jy, 1, True)
    add("inf=1 beside zero words", "identity_rule", zero, zero, 1, True)
    add("inf=0 with all-zero words", "identity_rule", zero, zero, 0, True)
    add("no inf array, zero words", "identity_rule", zero, zero, None, True)
    add("no inf array, non-zero words", "identity_rule", junk, jy, None, False)
    return tuple(cases)


# ----------------------------------------------------------------------------------------------------- (c) subgroup check
def curve_point_outside_subgroup(curve, group):
    """a point ON the curve whose order does not divide r (cofactor groups only): decompress small x values until one works"""
    oc = OC[curve]
    n = oser.fq_size(oc)
    G = Group(oc, group)
    x = 1
    while True:
        data = x.to_bytes(n, "little") + (b"" if group == 1 else (1).to_bytes(n, "little"))
        x += 1
        try:
            P = oser.point_decode(data, oc, group, checked=False)
        except oser.InvalidData:
            continue
        if P is not None and G.on_curve(P) and not oser.in_subgroup(P, oc, group):
            return P


def to_mont(curve, P):
    """(x, y) -> the Montgomery integers of its 2 or 4 base-field coordinates"""
    oc = OC[curve]
    flat = P if isinstance(P[0], int) else (*P[0], *P[1])
    return tuple(v * oc.fq_R % oc.q for v in flat)


def from_mont(curve, mont):
    oc = OC[curve]
    assert all(0 <= m < oc.q for m in mont)
    v = [m * pow(oc.fq_R, -1, oc.q) % oc.q for m in mont]
    return (v[0], v[1]) if len(v) == 2 else ((v[0], v[1]), (v[2], v[3]))


def bls_g1_order3_point():
    """T = (0, 2) on y^2 = x^3 + 4: 2 T = -T, and r = 1 (mod 3), so [r]T = T"""
    oc = OC["bls12_381"]
    G = Group(oc, 1)
    y = oser.sqrt_fp(oc.g1_b, oc.q)
    T = (0, min(y, oc.q - y))
    assert T == (0, 2) and G.on_curve(T) and G.add(T, T) == G.neg(T) and G.add(G.add(T, T), T) is None and oc.r % 3 == 1
    return T


@lru_cache(maxsize=None)
def subgroup_cases(curve, group):
    """BN254 G1 has cofactor 1: every curve point is in the subgroup, so it gets no low-order and no cofactor case; the control,
    off-curve and skipped-lane cases are generated for it as for the others."""
    oc = OC[curve]
    G = Group(oc, group)
    S = pool(curve, group)[17]
    cases = []

    def add(name, kind, mont, inf=0):
        if inf == 1 or not any(mont):
            want = True                                                              # a skipped lane
        else:
            P = from_mont(curve, mont)
            want = G.on_curve(P) and oser.in_subgroup(P, oc, group)
        cases.append(SubCase(name, kind, tuple(mont), inf, want))

    add("S (control)", "control", to_mont(curve, S))
    if (curve, group) == ("bls12_381", 1):
        T = bls_g1_order3_point()
        for nm, P in (("T=(0,2)", T), ("-T", G.neg(T)), ("S+T", G.add(S, T)), ("S-T", G.add(S, G.neg(T)))):
            add(nm, "low_order", to_mont(curve, P))
            assert G.on_curve(P) and cases[-1].want is False
    if (curve, group) != ("bn254", 1):
        Q = curve_point_outside_subgroup(curve, group)
        for nm, P in (("Q", Q), ("Q+S", G.add(Q, S)), ("-Q", G.neg(Q))):
            add(nm, "cofactor", to_mont(curve, P))
            assert G.on_curve(P) and cases[-1].want is False
    m = to_mont(curve, S)
    w = len(m)
    tweaks = [("y", w // 2), ("x", 0)] + ([("y.c1 only", w - 1), ("x.c1 only", 1)] if group == 2 else [])
    for nm, k in tweaks:
        t = list(m)
        t[k] ^= 1
        add(f"S with {nm} off by one in its lowest Montgomery word", "off_curve", t)
        assert cases[-1].want is False
    junk = list(m)
    junk[-1] ^= 1
    add("inf=1 beside off-curve words", "skipped", junk, 1)
    add("inf=1 beside zero words", "skipped", (0,) * w, 1)
    add("(0, 0) words, no inf array", "skipped", (0,) * w, None)
    add("(0, 0) words, inf=0", "skipped", (0,) * w, 0)
    assert cases[0].want is True
    return tuple(cases)


# ------------------------------------------------------------------------------------------------------ (d) the 64-lane grid
def failure_layouts():
    out = []
    for n in (1, 63, 64, 65, 128, 129, 193):
        for bad in ((n - 1,), (0,), (64, 63), (128, 65), (192, 65, 130)):
            if all(0 <= b < n for b in bad) and Layout(n, bad, min(bad)) not in out:
                out.append(Layout(n, bad, min(bad)))
    return out


def counts(cases):
    return dict(Counter(c.kind for c in cases))
