"""PLONK on the device: the composer (plonk/src/composer), AHPForPLONK::index (ahp/indexer/mod.rs:128-256) and prover rounds 1-3
(ahp/prover.rs:69-216), every table resident on the device.

The rounds produce every polynomial the prover commits: w_0..w_3, z and t_0..t_3.  A round is uploads, zkp_ntt_dev transforms
(interpolate = ifft over domain_n, then coset_fft over domain_4n of the zero-padded coefficients) and one fused call:
zkp_fr_plonk_perm_z_dev in round 2, zkp_fr_plonk_quotient_dev in round 3.  Commitments, openings and the transcript are the
caller's: the challenges beta, gamma and alpha are passed in.  Field elements are canonical Python integers; device tables are
Montgomery Fr.  A coefficient vector always has n entries (the reference drops trailing zeros).

After round 3 (Plonk::prove, plonk/src/lib.rs:93-204): prover_fourth_round evaluates the 20 coefficient vectors at zeta in ONE
zkp_fr_poly_eval_many_dev call (and z at zeta w in a second) and derives the eleven evaluations of
AHPForPLONK::construct_linear_combinations (ahp/mod.rs:29-113); prover_openings builds each opening polynomial with ONE
zkp_fr_lincomb_dev call and zkp_poly_div_linear_dev; prove() strings the rounds together with non-hiding KZG10 commitments and the
caller's transcript.  The Fiat-Shamir transcript of plonk/src/rng.rs and the verifier's pairing check are not here."""
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
FR_OPEN_MAX_POLYS = 32        # csrc/fr_open.hpp: vectors per zkp_fr_poly_eval_many_dev / zkp_fr_lincomb_dev call
FR_OPEN_EVAL_THREADS = 256    # the evaluation's grid is capped like the quotient's: THREADS * MAX_BLOCKS threads, each strides
FR_OPEN_EVAL_MAX_BLOCKS = 512
FR_OPEN_EVAL_GROUP = 4        # polynomials that share one walk of the powers of z (their accumulators stay in registers)

SELECTORS = ("q_0", "q_1", "q_2", "q_3", "q_m", "q_c", "q_arith", "sigma_0", "sigma_1", "sigma_2", "sigma_3")
PROVER_POLYS = ("w_0", "w_1", "w_2", "w_3", "z", "t_0", "t_1", "t_2", "t_3")     # AHPForPLONK::LABELS (ahp/mod.rs:26-27)
BASE_POLYS = PROVER_POLYS + SELECTORS                                            # the 20 vectors of n coefficients
# the eleven linear combinations in the order Plonk::prove sends their evaluations (lib.rs:171-183 sorts by label)
EVAL_LABELS = ("q_arith", "r", "sigma_0", "sigma_1", "sigma_2", "t", "w_0", "w_1", "w_2", "w_3", "z")
ZETA_LABELS = tuple(k for k in EVAL_LABELS if k != "z")                          # queried at zeta; z is queried at zeta w


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

    def __init__(self, ctx, curve, selectors: dict, ks, keep_coeffs: bool = False):
        """selectors: Composer.compose(ks), or the same keys with (n, 4) uint64 Montgomery arrays.  keep_coeffs: also keep the n
        coefficients of the 11 selector polynomials (coeffs[name]): rounds 4 and 5 evaluate and open them."""
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
        self.on_4n, self.sigma_n, self.coeffs = {}, [], {}
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
                if keep_coeffs:
                    self.coeffs[name] = self._alloc(self.n)
                extend_in_place(ctx, c, d, self.log_n, self.coeffs.get(name))
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
        self.on_4n, self.sigma_n, self.l1_4n, self.coeffs = {}, [], None, {}


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
        self.beta = self.gamma = self.alpha = self.zeta = None
        self.base_evals = self.evals = self.terms = None              # round 4: the 21 base evaluations, the eleven, r's terms
        self.open_tmp = self.w_zeta = self.w_shifted = None           # round 5 (allocated on first use)
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
    ps.alpha = alpha % c.r
    ps.round = 3
    names = [f"t_{k}" for k in range(4)]
    return [ps.read(k) for k in names] if to_host else [ps.coeffs[k] for k in names]


# ------------------------------------------------------------------------------- evaluations, linearisation, openings
def first_lagrange_at(n: int, zeta: int, r: int) -> int:
    """evaluate_first_lagrange_poly (utils.rs:45-50)"""
    return (pow(zeta, n, r) - 1) * pow(n * (zeta - 1), -1, r) % r


def linearisation_terms(curve, n: int, ks, base: dict, beta: int, gamma: int, alpha: int, zeta: int) -> list:
    """The eight (scalar, label) terms of r: ArithmeticKey::construct_linear_combination (indexer/arithmetic.rs:22-38) plus
    PermutationKey::construct_linear_combination (indexer/permutation.rs:32-65), signs as written there.  base: the evaluations
    of w_0..w_3, q_arith, sigma_0..sigma_2 at zeta and "z_shifted" = z(zeta w).  Host only."""
    r = get_curve(curve).r
    w = [base[f"w_{j}"] for j in range(4)]
    qa = base["q_arith"]
    terms = [(qa * w[0] % r, "q_0"), (qa * w[1] % r, "q_1"), (qa * w[2] % r, "q_2"), (qa * w[3] % r, "q_3"),
             (qa * w[1] % r * w[2] % r, "q_m"), (qa, "q_c")]
    numerator = 1
    for j in range(4):
        numerator = numerator * (w[j] + ks[j] * beta % r * zeta + gamma) % r
    denumerator = beta * base["z_shifted"] % r
    for j in range(3):
        denumerator = denumerator * (w[j] + beta * base[f"sigma_{j}"] + gamma) % r
    alpha_2 = alpha * alpha % r
    terms.append(((numerator * alpha + first_lagrange_at(n, zeta, r) * alpha_2) % r, "z"))
    terms.append((-denumerator * alpha % r, "sigma_3"))
    return terms


def prover_fourth_round(ps: ProverState, zeta: int) -> dict:
    """The evaluations Plonk::prove sends (lib.rs:143-183), keyed and ordered as EVAL_LABELS: ONE zkp_fr_poly_eval_many_dev call
    at zeta over the 20 base polynomials, one more for z at zeta w; t = sum zeta^(kn) t_k(zeta) and r(zeta) follow on the host by
    linearity.  The 21 base evaluations stay in ps.base_evals ("z_shifted": z at zeta w), r's terms in ps.terms."""
    ix, ctx, c = ps.index, ps.ctx, ps.index.curve
    assert ps.round >= 3
    if len(ix.coeffs) != len(SELECTORS):
        raise ValueError("round 4 needs the selector coefficients: build the Index with keep_coeffs=True")
    n, r = ix.n, c.r
    zeta %= r
    ptrs = [ps.coeffs[k] for k in PROVER_POLYS] + [ix.coeffs[k] for k in SELECTORS]
    at_zeta = fr_from_mont(ctx.fr_poly_eval_many_dev(c, ptrs, [n] * len(ptrs), fr_mont(zeta, c)), c)
    shifted = zeta * domain_generator(c, ix.log_n) % r
    base = dict(zip(BASE_POLYS, at_zeta))
    base["z_shifted"] = fr_from_mont(ctx.fr_poly_eval_many_dev(c, [ps.coeffs["z"]], [n], fr_mont(shifted, c)), c)[0]
    terms = linearisation_terms(c, n, ix.ks, base, ps.beta, ps.gamma, ps.alpha, zeta)
    zn = pow(zeta, n, r)
    evals = {k: base[k] for k in EVAL_LABELS if k in base}
    evals["z"] = base["z_shifted"]
    evals["t"] = sum(pow(zn, k, r) * base[f"t_{k}"] for k in range(4)) % r
    evals["r"] = sum(s * base[label] for s, label in terms) % r
    ps.zeta, ps.base_evals, ps.terms = zeta, base, terms
    ps.evals = {k: evals[k] for k in EVAL_LABELS}
    ps.round = 4
    return dict(ps.evals)


def _lincomb(ps: ProverState, terms, out_ptr: int):
    """out = sum scalar * polynomial(label) over n coefficients: ONE zkp_fr_lincomb_dev call"""
    ix, c = ps.index, ps.index.curve
    at = lambda label: ps.coeffs[label] if label in ps.coeffs else ix.coeffs[label]      # noqa: E731
    ps.ctx.fr_lincomb_dev(c, [at(label) for _, label in terms], [ix.n] * len(terms), fr_to_mont([s % c.r for s, _ in terms], c), out_ptr,
                          ix.n)


def linearisation_poly(ps: ProverState, terms, out_ptr: int):
    """the n coefficients of r = sum scalar * label (terms: linearisation_terms) into out_ptr, one zkp_fr_lincomb_dev call"""
    if len(ps.index.coeffs) != len(SELECTORS):
        raise ValueError("the linearisation polynomial needs the selector coefficients: build the Index with keep_coeffs=True")
    _lincomb(ps, terms, out_ptr)


def verifier_equality_check(curve, n: int, evals: dict, public_inputs, beta: int, gamma: int, alpha: int, zeta: int) -> bool:
    """verifier_equality_check (ahp/verifier.rs:101-150) on the eleven evaluations.  pi(zeta) is taken in Lagrange form over the
    non-zero public inputs: sum pi_i w^i (zeta^n - 1) / (n (zeta - w^i)).  Host only."""
    c = get_curve(curve)
    r = c.r
    v_zeta = (pow(zeta, n, r) - 1) % r
    w = domain_generator(c, n.bit_length() - 1)
    pi_zeta, wi = 0, 1
    for v in public_inputs:
        if v % r:
            pi_zeta += v * wi % r * v_zeta % r * pow(n * (zeta - wi), -1, r)
        wi = wi * w % r
    prod = evals["z"] * (evals["w_3"] + gamma) % r
    for j in range(3):
        prod = prod * (evals[f"w_{j}"] + beta * evals[f"sigma_{j}"] + gamma) % r
    lhs = evals["t"] * v_zeta % r
    rhs = (evals["r"] + evals["q_arith"] * pi_zeta - prod * alpha - first_lagrange_at(n, zeta, r) * alpha * alpha) % r
    return lhs == rhs


def opening_weights(curve, epsilon: int) -> dict:
    """epsilon^j over the labels queried at zeta in ascending order, starting at epsilon^0: how ark-poly-commit 0.2's
    open_combinations batches the linear combinations of one point [recalled, unverifiable offline: the crate is not in the
    reference tree]"""
    r = get_curve(curve).r
    return {label: pow(epsilon, j, r) for j, label in enumerate(ZETA_LABELS)}


def zeta_opening_terms(ps: ProverState, weights: dict) -> list:
    """sum_label weights[label] * LC_label over ZETA_LABELS as (scalar, base polynomial) terms: the LCs t and r are expanded into
    their terms, so each of the 20 base polynomials appears once and no LC polynomial is materialised"""
    r, n = ps.index.curve.r, ps.index.n
    zn = pow(ps.zeta, n, r)
    acc = dict.fromkeys(BASE_POLYS, 0)
    for label in ZETA_LABELS:
        wgt = weights[label] % r
        if label == "t":
            for k in range(4):
                acc[f"t_{k}"] += wgt * pow(zn, k, r)
        elif label == "r":
            for s, name in ps.terms:
                acc[name] += wgt * s
        else:
            acc[label] += wgt
    return [(acc[k] % r, k) for k in BASE_POLYS]


def prover_openings(ps: ProverState, zeta: int, weights: dict | None = None, epsilon: int | None = None, to_host: bool = True):
    """The two opening polynomials of PC::open_combinations for verifier_query_set (ahp/verifier.rs:77-99):
        W_zeta = (sum_label weights[label] * LC_label) / (X - zeta)  over the ten labels queried at zeta (ZETA_LABELS),
        W_shifted_zeta = z / (X - zeta w).
    W_zeta is ONE zkp_fr_lincomb_dev call over the 20 base polynomials (zeta_opening_terms), then zkp_poly_div_linear_dev;
    W_shifted_zeta divides z directly.  Each has n - 1 coefficients and stays on the device (ps.w_zeta, ps.w_shifted).
    weights: label -> integer.  Without weights, epsilon gives opening_weights(): epsilon^j over the labels in ascending order
    from epsilon^0, as ark-poly-commit 0.2's open_combinations does [recalled, unverifiable offline].
    Returns (W_zeta, W_shifted_zeta) as coefficient lists (to_host) or device pointers."""
    ix, ctx, c = ps.index, ps.ctx, ps.index.curve
    assert ps.round >= 4 and zeta % c.r == ps.zeta
    if weights is None:
        if epsilon is None:
            raise ValueError("weights or epsilon")
        weights = opening_weights(c, epsilon)
    n = ix.n
    if ps.open_tmp is None:
        ps.open_tmp, ps.w_zeta, ps.w_shifted = ps._alloc(n), ps._alloc(n), ps._alloc(n)
    _lincomb(ps, zeta_opening_terms(ps, weights), ps.open_tmp)
    ctx.poly_div_linear(c, ps.open_tmp, n, fr_mont(ps.zeta, c), ps.w_zeta)
    ctx.poly_div_linear(c, ps.coeffs["z"], n, fr_mont(ps.zeta * domain_generator(c, ix.log_n) % c.r, c), ps.w_shifted)
    ps.round = 5
    if not to_host:
        return ps.w_zeta, ps.w_shifted
    out = []
    for d in (ps.w_zeta, ps.w_shifted):
        a = np.zeros((n - 1, 4), dtype=np.uint64)
        ctx.d2h(a, d)
        out.append(fr_from_mont(a, c))
    return tuple(out)


def _commit(ctx, ck, c, d: int, count: int):
    """non-hiding KZG10 commitment to `count` coefficients on the device (to_labeled, utils.rs:61-63: no hiding bound, no
    degree bound) as an affine canonical point (None: the identity)"""
    from .codec import g1_from_mont
    xy, inf = ctx.into_affine(c, 1, ck.powers_of_g.msm_mont_dev(d, count))
    return g1_from_mont(xy, [inf], c)[0]


def prove(ctx, ck, index: Index, witnesses, public_inputs, challenge) -> dict:
    """Plonk::prove (lib.rs:93-204) without its transcript: rounds 1-3, the commitments, round 4 and the openings.
    ck: a kzg10.CommitterKey with at least n powers.  challenge(stage, payload) is the caller's transcript: stage 1 -> (beta, gamma)
    after the commitments to w_0..w_3, 2 -> alpha after z, 3 -> zeta after t_0..t_3 (payload: the commitments so far), 4 -> epsilon
    after the evaluations (payload: the evaluations).  Returns {"commitments": label -> point for the nine prover polynomials,
    "evaluations": the eleven in the reference's order, "witnesses": (commitment to W_zeta, to W_shifted_zeta)}; points are affine
    canonical (x, y), None for the identity."""
    c, n = index.curve, index.n
    if ck.supported_degree + 1 < n:
        raise ValueError("the committer key has fewer than n powers")
    ps = prover_init(index, public_inputs)
    try:
        comms = {}
        for k, d in zip(PROVER_POLYS[:4], prover_first_round(ps, witnesses, to_host=False)):
            comms[k] = _commit(ctx, ck, c, d, n)
        beta, gamma = challenge(1, dict(comms))
        comms["z"] = _commit(ctx, ck, c, prover_second_round(ps, beta, gamma, to_host=False), n)
        alpha = challenge(2, dict(comms))
        for k, d in zip(PROVER_POLYS[5:], prover_third_round(ps, alpha, to_host=False)):
            comms[k] = _commit(ctx, ck, c, d, n)
        zeta = challenge(3, dict(comms))
        evals = prover_fourth_round(ps, zeta)
        epsilon = challenge(4, dict(evals))
        w_zeta, w_shifted = prover_openings(ps, zeta, epsilon=epsilon, to_host=False)
        wit = (_commit(ctx, ck, c, w_zeta, n - 1), _commit(ctx, ck, c, w_shifted, n - 1))
    finally:
        ps.close()
    return {"commitments": comms, "evaluations": evals, "witnesses": wit}
