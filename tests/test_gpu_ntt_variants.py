"""Every NTT kernel variant, pass plan and fused chain of csrc/ntt.hip on small domains (DESIGN.md §NTT lists which case covers what).

The default configuration at 2^12 (two passes of even S, full tables) is what the rest of the suite runs.  Here:
  * one child process per switch setting (tests/ntt_variant_child.py): the legacy pass kernel with its radix-2 tail stage, the
    two-level twiddle / coset lookups, batched transforms, odd pass counts of three and five (ZKP_NTT_SMAX=4 makes 2^9 a three-pass
    and 2^17 a five-pass transform), S = 10 tiles, the fused witness-map chains and their fallbacks — both scalar fields, against
    oracle/cpu, word for word;
  * in this process, with the default switches: every log_n 0..19 against oracle/cpu and (<= 2^12) the Python-integer reference, the
    closed form of a unit vector's transform, zkp_ntt_dev between guard regions, every build order of the lazily built tables, and
    the argument rules of both entry points."""
import ctypes as C

import numpy as np
import pytest

from ckb_zkp_amd import api, codec
from ckb_zkp_amd.params import get_curve
from oracle import cpu_oracle
from oracle.pyref.ntt import Domain
from tests import ntt_variant_child as nv
from tests.util import OC

pytestmark = pytest.mark.gpu
CURVES = list(nv.CURVES)
OP_NAMES = {api.NTT_FFT: "fft", api.NTT_IFFT: "ifft", api.NTT_COSET_FFT: "coset_fft", api.NTT_COSET_IFFT: "coset_ifft"}


def _r(a, b):
    return list(range(a, b + 1))


@pytest.mark.parametrize("switches,log_ns,ks", [pytest.param(*v[1:], id=v[0]) for v in nv.VARIANTS])
def test_variant_in_its_own_process(switches, log_ns, ks):
    """Children run strictly one after another (this process holds the GPU too: at most two at a time)."""
    spec = {"ntt": log_ns, "witness": ks}
    res = nv.run_variant(switches, spec)
    print(switches, "checked", res["checked"])


# ------------------------------------------------------------------------------------------------ in process, default switches
_ORACLE = {}          # (curve, log_n, op) -> oracle/cpu's transform of the `uniform` input: computed once, shared, never modified


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _ORACLE.clear()


def _reference(curve, log_n, name, x, op):
    if name != "uniform":
        return cpu_oracle.ntt(OC[curve].cid, x, op, threads=8)
    key = (curve, log_n, op)
    if key not in _ORACLE:
        _ORACLE[key] = cpu_oracle.ntt(OC[curve].cid, x, op, threads=8)
        _ORACLE[key].setflags(write=False)
    return _ORACLE[key]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", _r(0, 19))
def test_every_size_matches_both_references(ctx, curve, log_n):
    """No size is left to chance: 2^0 .. 2^19 (one, two and three passes of the default plan), all four ops, every input of
    ntt_variant_child.inputs; up to 2^12 also against oracle/pyref (Python integers, independent of oracle/cpu)."""
    c = get_curve(curve)
    dom = Domain(OC[curve], 1 << log_n) if log_n <= 12 else None
    for name, x in nv.inputs(curve, log_n):
        xi = codec.fr_from_mont(x, c) if dom else None
        for op in nv.OPS:
            got = ctx.ntt(c, x, op)
            assert nv.first_bad(got, _reference(curve, log_n, name, x, op)) == -1, (curve, log_n, name, op)
            if dom:
                assert codec.fr_from_mont(got, c) == getattr(dom, OP_NAMES[op])(xi), (curve, log_n, name, op, "pyref")


@pytest.mark.parametrize("curve", CURVES)
def test_three_passes_with_more_workgroups_than_the_device_holds(ctx, curve):
    """2^21 = 7 + 7 + 7: 2048 workgroups per pass on 1024 resident slots (four per CU).  Up to 2^19 every workgroup of a pass is
    resident at once and has loaded its tile before any of them stores, so a pass that read and wrote the SAME buffer would still
    come out right; the two scratch halves of an odd pass count (s0 -> s1 -> data) only matter from here on
    (profiles/ntt_variant_tests.txt, mutation d).  The one case above the 16 MiB the rest of this file stays under."""
    log_n = 21
    assert nv.plan(log_n) == [7, 7, 7]
    x = nv.make_input(curve, log_n, "uniform")
    for op in nv.OPS:
        got = ctx.ntt(curve, x, op)
        assert nv.first_bad(got, cpu_oracle.ntt(OC[curve].cid, x, op, threads=8)) == -1, (curve, op)
        del got


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", _r(1, nv.UNIT_MAX_LOG))
def test_unit_vector_closed_form(ctx, curve, log_n):
    """x = e_j: fft(x)[i] = w^(ij) and coset_fft(x)[i] = (g w^i)^j, from Python's pow alone (no oracle).  The j sit on the row
    boundaries of the first pass's tile."""
    c = get_curve(curve)
    n, r = 1 << log_n, c.r
    w = pow(pow(c.fr_generator, (r - 1) >> c.two_adicity, r), 1 << (c.two_adicity - log_n), r)
    for j in nv.unit_positions(log_n):
        x = nv.make_input(curve, log_n, f"unit{j}")
        wj, gj = pow(w, j, r), pow(c.fr_generator, j, r)
        col, p = [], 1
        for _ in range(n):                                            # w^(ij), i = 0 .. N - 1
            col.append(p)
            p = p * wj % r
        assert p == 1 and col[1 % n] == pow(w, j * (1 % n), r) and col[n - 1] == pow(w, j * (n - 1), r)
        assert nv.first_bad(ctx.ntt(c, x, api.NTT_FFT), codec.fr_to_mont(col, c)) == -1, (curve, log_n, j, "fft")
        assert nv.first_bad(ctx.ntt(c, x, api.NTT_COSET_FFT), codec.fr_to_mont([gj * v % r for v in col], c)) == -1, \
            (curve, log_n, j, "coset_fft")


GUARD = 64
SENTINEL = np.uint64(0xA5C3A5C3A5C3A5C3)


class _Guarded:
    """a device buffer of GUARD + n + GUARD Fr elements filled with a sentinel; `mid` points at the middle n"""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.host = np.full((n + 2 * GUARD, 4), SENTINEL, dtype=np.uint64)
        self.dev = ctx.to_device(self.host)
        self.mid = self.dev + GUARD * 32

    def read(self):
        out = np.zeros_like(self.host)
        self.ctx.d2h(out, self.dev)
        return out

    def guards_intact(self, buf):
        return bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + self.n:] == SENTINEL).all())

    def free(self):
        self.ctx.dev_free(self.dev)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("log_n", [0, 1, 9, 10, 13, 19])
def test_ntt_dev_between_guards(ctx, curve, log_n):
    """zkp_ntt_dev in place on the middle of a larger buffer: the result is the host entry point's, nothing outside the N elements
    is written — one pass (2^9: via scratch and a copy), two, and three (2^19: both scratch halves) — and the same buffer takes the
    next op as well."""
    c = get_curve(curve)
    n = 1 << log_n
    g = _Guarded(ctx, n)
    try:
        cur = nv.make_input(curve, log_n, "uniform")
        ctx.h2d(g.mid, cur)
        for op in (api.NTT_COSET_FFT, api.NTT_IFFT, api.NTT_FFT, api.NTT_COSET_IFFT):
            ctx.ntt_dev(c, g.mid, log_n, op)
            ctx.sync()
            buf = g.read()
            cur = ctx.ntt(c, cur, op)
            assert g.guards_intact(buf), (curve, log_n, op)
            assert nv.first_bad(buf[GUARD:GUARD + n], cur) == -1, (curve, log_n, op)
    finally:
        g.free()


@pytest.mark.parametrize("log_n", [11, 19])
def test_table_build_order(ctx, log_n):
    """The per-key tables (inter-pass twiddles per direction and pass, the two coset tables) are built on first use.  The suite
    always asks for the forward transform first; here context i starts with op i, and a fifth context alternates the two fields."""
    from ckb_zkp_amd.api import Context
    x = {curve: nv.make_input(curve, log_n, "uniform") for curve in CURVES}
    for first in nv.OPS:
        with Context(ctx.device) as fresh:
            for curve in CURVES:
                for op in [first] + [o for o in nv.OPS if o != first]:
                    got = fresh.ntt(curve, x[curve], op)
                    assert nv.first_bad(got, _reference(curve, log_n, "uniform", x[curve], op)) == -1, (first, curve, op)
    with Context(ctx.device) as fresh:
        for op in (api.NTT_COSET_IFFT, api.NTT_FFT, api.NTT_COSET_FFT, api.NTT_IFFT):
            for curve in CURVES + CURVES:
                got = fresh.ntt(curve, x[curve], op)
                assert nv.first_bad(got, _reference(curve, log_n, "uniform", x[curve], op)) == -1, ("alternating", curve, op)


@pytest.mark.parametrize("cid,log_n,op,status", [
    (0, 3, 4, -1), (0, 3, -1, -1), (1, 3, 4, -1), (1, 3, -1, -1),          # op out of range -> ZKP_ERR_BAD_ARG
    (7, 3, 0, -2),                                                          # unknown curve -> ZKP_ERR_UNSUPPORTED_CURVE
    (0, 29, 0, -3), (1, 31, 0, -3), (1, 33, 0, -3)])                        # above the cap -> ZKP_ERR_DOMAIN_TOO_LARGE
def test_argument_rules(ctx, cid, log_n, op, status):
    """Both entry points refuse with the same status and touch neither the host array nor the device buffer.  (The arrays hold 8
    elements whatever log_n claims: a refused call must not read or write a single one.)"""
    n = 8
    host = np.full((n, 4), SENTINEL, dtype=np.uint64)
    assert ctx.lib.zkp_ntt(ctx.h, cid, C.c_void_p(host.ctypes.data), log_n, op) == status
    assert (host == SENTINEL).all()
    g = _Guarded(ctx, n)
    try:
        assert ctx.lib.zkp_ntt_dev(ctx.h, cid, C.c_void_p(g.mid), log_n, op) == status
        ctx.sync()
        assert (g.read() == SENTINEL).all()
    finally:
        g.free()
    # the context is still good
    x = nv.make_input("bn254", 3, "uniform")
    assert nv.first_bad(ctx.ntt("bn254", x, api.NTT_FFT), cpu_oracle.ntt(0, x, api.NTT_FFT)) == -1
