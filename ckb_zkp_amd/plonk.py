"""PLONK on the device: the composer (plonk/src/composer), AHPForPLONK::index (ahp/indexer/mod.rs:128-256) and prover rounds 1-3
(ahp/prover.rs:69-216), every table resident on the device.

The rounds produce every polynomial the prover commits: w_0..w_3, z and t_0..t_3.  A round is uploads, zkp_ntt_dev transforms
(interpolate = ifft over domain_n, then coset_fft over domain_4n of the zero-padded coefficients) and one fused call:
zkp_fr_plonk_perm_z_dev in round 2, zkp_fr_plonk_quotient_dev in round 3.  Commitments, openings and the transcript are the
caller's: the challenges beta, gamma and alpha are passed in.  Field elements are canonical Python integers; device tables are
Montgomery Fr.  A coefficient vector always has n entries (the reference drops trailing zeros)."""
from __future__ import annotations

import numpy as np

from .api import NTT_COSET_FFT, NTT_COSET_IFFT, NTT_IFFT
from .codec import fr_from_mont, fr_mont, fr_to_mont
from .params import get_curve

PLONK_SCAN_THREADS = 256      # csrc/plonk.hpp: threads of a running-product workgroup
PLONK_SCAN_ITEMS = 4          # elements per thread
PLONK_SCAN_BLOCK = 1024       # elements per workgroup; more than one block: the totals are scanned as a level of their own
PLONK_QUOT_THREADS = 256      # the quotient kernel's grid is capped at THREADS * MAX_BLOCKS threads; each strides over its points
PLONK_QUOT_MAX_BLOCKS = 512

SELECTORS = ("q_0", "q_1", "q_2", "q_3", "q_m", "q_c", "q_arith", "sigma_0", "sigma_1", "sigma_2", "sigma_3")


def domain_generator(curve, log_n: int) -> int:
    """domain.element(1) of the radix-2 domain of size 2^log_n: the root zkp_ntt_dev uses"""
    c = get_curve(curve)
    if log_n > c.two_adicity:
        raise ValueError("PolynomialDegreeTooLarge")
    root = pow(c.fr_generator, (c.r - 1) >> c.two_adicity, c.r)
    return pow(root, 1 << (c.two_adicity - log_n), c.r)


def _log2_ceil(n: int) -> int:
    return (max(n, 1) - 1).bit_length()


class Composer:
    """composer/mod.rs, arithmetic.rs, permutation.rs, synthesize.rs.  A variable is its index; variable 0 is null_var (value 0).
    A gate's wires are (aux, l, r, o) = w_0..w_3 and it states  q_0 aux + q_1 l + q_2 r + q_3 o + q_m l r + q_c + pi = 0."""

    def __init__(self, curve):
        self.curve = get_curve(curve)
        self.r = self.curve.r
        self.n = 0
        self.q = {k: [] for k in SELECTORS[:7]}
        self.pi = []
        self.w = [[], [], [], []]
        self.wires = []                    # variable -> [(wire, gate)]: Permutation::variable_map
        self.assignment = []
        self.null_var = self.alloc_and_assign(0)

    def size(self) -> int:
        return self.n

    def alloc_and_assign(self, value: int) -> int:
        self.wires.append([])
        self.assignment.append(value % self.r)
        return len(self.assignment) - 1

    def _create_poly_gate(self, l, r, o, aux, q_m, q_c, pi):
        aux = (self.null_var, 0) if aux is None else aux
        for j, (var, coeff) in enumerate((aux, l, r, o)):
            self.wires[var].append((j, self.n))
            self.w[j].append(var)
            self.q[SELECTORS[j]].append(coeff % self.r)
        self.q["q_m"].append(q_m % self.r)
        self.q["q_c"].append(q_c % self.r)
        self.q["q_arith"].append(1)
        self.pi.append(pi % self.r)
        self.n += 1

    def constrain_to_constant(self, var: int, value: int, pi: int = 0):
        self._create_poly_gate((var, 1), (var, 0), (var, 0), None, 0, -value, -pi)

    def assert_equal(self, l: int, r: int):
        self._create_poly_gate((l, 1), (r, -1), (self.null_var, 0), None, 0, 0, 0)

    def create_add_gate(self, l, r, o: int, aux=None, q_c: int = 0, pi: int = 0):
        """l, r, aux: (variable, coefficient)"""
        self._create_poly_gate(l, r, (o, -1), aux, 0, q_c, pi)

    def create_mul_gate(self, l: int, r: int, o: int, aux=None, q_m: int = 1, q_c: int = 0, pi: int = 0):
        self._create_poly_gate((l, 0), (r, 0), (o, -1), aux, q_m, q_c, pi)

    def domain_size(self) -> int:
        return 1 << _log2_ceil(self.n)

    def compose(self, ks) -> dict:
        """Selectors: the 7 selector vectors zero-padded to n = domain_size() and sigma_0..sigma_3 (compute_sigmas)"""
        n, r = self.domain_size(), self.r
        w = domain_generator(self.curve, _log2_ceil(n))
        roots = [1] * n
        for i in range(1, n):
            roots[i] = roots[i - 1] * w % r
        perm = [[(j, i) for i in range(n)] for j in range(4)]        # compute_wire_permutation
        for wires in self.wires:
            if len(wires) <= 1:
                continue
            for cur, (j, i) in enumerate(wires):
                perm[j][i] = wires[cur - 1]                           # cur == 0: the last one
        out = {k: v + [0] * (n - self.n) for k, v in self.q.items()}
        for j in range(4):
            out[f"sigma_{j}"] = [roots[i] * (ks[jj] % r) % r for jj, i in perm[j]]
        out["n"] = n
        return out

    def public_inputs(self) -> list:
        return list(self.pi)

    def synthesize(self) -> list:
        """Witnesses: w_0..w_3 zero-padded to n"""
        pad = [0] * (self.domain_size() - self.n)
        return [[self.assignment[v] for v in col] + pad for col in self.w]


class Index:
    """AHPForPLONK::index on the device: the 11 selector vectors over the 4n coset (ifft over domain_n, coset_fft over domain_4n),
    sigma_0..sigma_3 over domain_n (compute_z reads them) and l1_4n.  close() frees every buffer."""

    def __init__(self, ctx, curve, selectors: dict, ks):
        """selectors: Composer.compose(ks), or the same keys with (n, 4) uint64 Montgomery arrays"""
        self.ctx, self.curve = ctx, get_curve(curve)
        c = self.curve
        self.ks = [k % c.r for k in ks]
        self.n = int(selectors["n"])
        if self.n < 4 or self.n & (self.n - 1):
            raise ValueError("n must be a power of two, at least 4")
        self.log_n = self.n.bit_length() - 1
        if self.log_n + 2 > c.two_adicity:
            raise ValueError("PolynomialDegreeTooLarge")
        self.bufs = []
        self.on_4n, self.sigma_n = {}, []
        try:
            for name in SELECTORS:
                evals = _as_mont(selectors[name], c)
                assert evals.shape == (self.n, 4), name
                d = self._alloc(4 * self.n)
                ctx.h2d(d, evals)
                if name.startswith("sigma"):
                    keep = self._alloc(self.n)
                    ctx.d2d(keep, d, 32 * self.n)
                    self.sigma_n.append(keep)
                extend_in_place(ctx, c, d, self.log_n)
                self.on_4n[name] = d
            l1 = np.zeros((self.n, 4), dtype=np.uint64)                # first_lagrange_poly (utils.rs:39-43)
            l1[0] = fr_mont(1, c)
            self.l1_4n = self._alloc(4 * self.n)
            ctx.h2d(self.l1_4n, l1)
            extend_in_place(ctx, c, self.l1_4n, self.log_n)
            ctx.sync()
        except Exception:
            self.close()
            raise

    def _alloc(self, elems: int) -> int:
        d = self.ctx.dev_alloc(32 * elems)
        self.bufs.append(d)
        return d

    def q_ptrs(self):
        return [self.on_4n[k] for k in SELECTORS[:7]]

    def sigma_ptrs(self):
        return [self.on_4n[k] for k in SELECTORS[7:]]

    def close(self):
        bufs, self.bufs = self.bufs, []
        if bufs:
            self.ctx.sync()
        for d in bufs:
            self.ctx.dev_free(d)
        self.on_4n, self.sigma_n, self.l1_4n = {}, [], None


def _as_mont(v, c) -> np.ndarray:
    if isinstance(v, np.ndarray) and v.dtype == np.uint64:
        return np.ascontiguousarray(v)
    return fr_to_mont(v, c)


def extend_in_place(ctx, c, d: int, log_n: int, coeffs_out: int | None = None):
    """d: 4n Fr on the device with evaluations over domain_n in the first n.  Interpolates them in place, optionally copies the n
    coefficients to coeffs_out, zero-pads to 4n (zkp_dev_zero) and evaluates over the coset of domain_4n."""
    n = 1 << log_n
    ctx.ntt_dev(c, d, log_n, NTT_IFFT)
    if coeffs_out is not None:
        ctx.d2d(coeffs_out, d, 32 * n)
    ctx.dev_zero(d + 32 * n, 32 * 3 * n)
    ctx.ntt_dev(c, d, log_n + 2, NTT_COSET_FFT)


class ProverState:
    """ProverState of ahp/prover.rs:17-30 with every vector on the device.  coeffs[name]: device pointer to the n coefficients
    of w_0..w_3, z, t_0..t_3 once their round has run (valid until close())."""

    def __init__(self, index: Index):
        self.index, self.ctx = index, index.ctx
        n = index.n
        self.bufs = []
        self.pi_4n = self._alloc(4 * n)
        self.w_n = [self._alloc(n) for _ in range(4)]
        self.w_4n = [self._alloc(4 * n) for _ in range(4)]
        self.z_4n = self._alloc(4 * n)
        self.t = self._alloc(4 * n)
        w_coeffs = [self._alloc(n) for _ in range(4)]
        self.coeffs = {f"w_{j}": w_coeffs[j] for j in range(4)}
        self.coeffs["z"] = self._alloc(n)
        for k in range(4):
            self.coeffs[f"t_{k}"] = self.t + 32 * n * k               # quad_split: consecutive chunks of n coefficients
        self.beta = self.gamma = None
        self.round = 0

    def _alloc(self, elems: int) -> int:
        d = self.ctx.dev_alloc(32 * elems)
        self.bufs.append(d)
        return d

    def read(self, name: str) -> list:
        """a coefficient vector as integers"""
        a = np.zeros((self.index.n, 4), dtype=np.uint64)
        self.ctx.d2h(a, self.coeffs[name])
        return fr_from_mont(a, self.index.curve)

    def close(self):
        bufs, self.bufs = self.bufs, []
        if bufs:
            self.ctx.sync()
        for d in bufs:
            self.ctx.dev_free(d)


def prover_init(index: Index, public_inputs) -> ProverState:
    """prover_init (prover.rs:69-95): pi_4n.  public_inputs: Composer.public_inputs() (at most n values), or (n, 4) Montgomery"""
    c, n = index.curve, index.n
    ps = ProverState(index)
    try:
        pi = public_inputs if isinstance(public_inputs, np.ndarray) else fr_to_mont(list(public_inputs) + [0] * (n - len(public_inputs)), c)
        assert pi.shape == (n, 4)
        ps.ctx.h2d(ps.pi_4n, pi)
        extend_in_place(ps.ctx, c, ps.pi_4n, index.log_n)
    except Exception:
        ps.close()
        raise
    return ps


def prover_first_round(ps: ProverState, witnesses, to_host: bool = True):
    """prover_first_round (prover.rs:97-133).  witnesses: Composer.synthesize(), or 4 (n, 4) Montgomery arrays.
    Returns w_0..w_3 as coefficient lists (to_host) or device pointers."""
    ix, ctx = ps.index, ps.ctx
    assert len(witnesses) == 4
    for j in range(4):
        w = _as_mont(witnesses[j], ix.curve)
        assert w.shape == (ix.n, 4)
        ctx.h2d(ps.w_n[j], w)
        ctx.d2d(ps.w_4n[j], ps.w_n[j], 32 * ix.n)
        extend_in_place(ctx, ix.curve, ps.w_4n[j], ix.log_n, ps.coeffs[f"w_{j}"])
    ps.round = 1
    names = [f"w_{j}" for j in range(4)]
    return [ps.read(k) for k in names] if to_host else [ps.coeffs[k] for k in names]


def prover_second_round(ps: ProverState, beta: int, gamma: int, to_host: bool = True):
    """prover_second_round (prover.rs:135-165): z.  Raises ValueError where the reference's assert_eq! fails
    (indexer/permutation.rs:112): the witness does not satisfy the copy constraints."""
    ix, ctx, c = ps.index, ps.ctx, ps.index.curve
    assert ps.round >= 1
    ps.beta, ps.gamma = beta % c.r, gamma % c.r
    closes = ctx.fr_plonk_perm_z_dev(c, ps.w_n, ix.sigma_n, ix.log_n, fr_to_mont(ix.ks, c), fr_mont(ps.beta, c), fr_mont(ps.gamma, c),
                                     ps.z_4n)
    if not closes:
        raise ValueError("the permutation accumulator does not close: z[n-1] * perm[n-1] != 1")
    extend_in_place(ctx, c, ps.z_4n, ix.log_n, ps.coeffs["z"])
    ps.round = 2
    return ps.read("z") if to_host else ps.coeffs["z"]


def prover_third_round(ps: ProverState, alpha: int, to_host: bool = True):
    """prover_third_round (prover.rs:167-216): t = (t_arith + t_perm) / v over the 4n coset, coset_ifft, quad_split -> t_0..t_3"""
    ix, ctx, c = ps.index, ps.ctx, ps.index.curve
    assert ps.round >= 2
    ctx.fr_plonk_quotient_dev(c, ps.w_4n, ps.z_4n, ps.pi_4n, ix.q_ptrs(), ix.sigma_ptrs(), ix.l1_4n, ix.log_n, fr_to_mont(ix.ks, c),
                              fr_mont(ps.beta, c), fr_mont(ps.gamma, c), fr_mont(alpha % c.r, c), ps.t)
    ctx.ntt_dev(c, ps.t, ix.log_n + 2, NTT_COSET_IFFT)
    ps.round = 3
    names = [f"t_{k}" for k in range(4)]
    return [ps.read(k) for k in names] if to_host else [ps.coeffs[k] for k in names]
