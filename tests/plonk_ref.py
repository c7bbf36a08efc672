"""REFERENCE (test infrastructure only): PLONK's composer, indexer and prover rounds 1-3 in Python integers, written from
plonk/src/composer/{mod,arithmetic,permutation,synthesize}.rs, plonk/src/ahp/indexer/{mod,arithmetic,permutation}.rs and
plonk/src/ahp/prover.rs.  Transforms are oracle/pyref/ntt.py's Domain.  Values are canonical integers mod r; nothing here shares
code with ckb_zkp_amd/plonk.py."""
from oracle.pyref.fields import CURVES
from oracle.pyref.ntt import Domain

WIRES = 4
Q_NAMES = ("q_0", "q_1", "q_2", "q_3", "q_m", "q_c", "q_arith")
S_NAMES = ("sigma_0", "sigma_1", "sigma_2", "sigma_3")


class RefComposer:
    """gates: rows (aux, l, r, o | q_0, q_1, q_2, q_3, q_m, q_c | pi); variable 0 is null_var with value 0 (mod.rs:66)"""

    def __init__(self, curve):
        self.curve = CURVES[curve]
        self.r = self.curve.r
        self.values = [0]
        self.rows = []

    def alloc_and_assign(self, value):
        self.values.append(value % self.r)
        return len(self.values) - 1

    def poly_gate(self, l, r, o, aux, q_m, q_c, pi):                 # arithmetic.rs:5-41
        aux = aux if aux is not None else (0, 0)
        m = self.r
        self.rows.append(((aux[0], l[0], r[0], o[0]), (aux[1] % m, l[1] % m, r[1] % m, o[1] % m, q_m % m, q_c % m), pi % m))

    def constrain_to_constant(self, var, value, pi=0):               # :43-53
        self.poly_gate((var, 1), (var, 0), (var, 0), None, 0, -value, -pi)

    def assert_equal(self, l, r):                                    # :55-65
        self.poly_gate((l, 1), (r, -1), (0, 0), None, 0, 0, 0)

    def create_add_gate(self, l, r, o, aux=None, q_c=0, pi=0):       # :67-77
        self.poly_gate(l, r, (o, -1), aux, 0, q_c, pi)

    def create_mul_gate(self, l, r, o, aux=None, q_m=1, q_c=0, pi=0):   # :79-102
        self.poly_gate((l, 0), (r, 0), (o, -1), aux, q_m, q_c, pi)

    def size(self):
        return len(self.rows)

    def domain(self):
        return Domain(self.curve, len(self.rows))

    def roots(self):
        d = self.domain()
        out, x = [], 1
        for _ in range(d.size):
            out.append(x)
            x = x * d.group_gen % self.r
        return out

    def compose(self, ks):
        """synthesize.rs:69-108 with compute_sigmas / compute_wire_permutation (permutation.rs:62-118)"""
        n, r, roots = self.domain().size, self.r, self.roots()
        sel = {"n": n}
        for k, name in enumerate(Q_NAMES[:6]):
            sel[name] = [row[1][k] for row in self.rows] + [0] * (n - len(self.rows))
        sel["q_arith"] = [1] * len(self.rows) + [0] * (n - len(self.rows))
        uses = {}
        for g, row in enumerate(self.rows):
            for col, var in enumerate(row[0]):
                uses.setdefault(var, []).append((col, g))
        target = {(col, g): (col, g) for col in range(WIRES) for g in range(n)}
        for cycle in uses.values():
            if len(cycle) > 1:
                for pos, wire in enumerate(cycle):
                    target[wire] = cycle[pos - 1] if pos else cycle[-1]
        for col, name in enumerate(S_NAMES):
            sel[name] = [roots[target[(col, g)][1]] * ks[target[(col, g)][0]] % r for g in range(n)]
        return sel

    def public_inputs(self):
        return [row[2] for row in self.rows]

    def synthesize(self):                                            # synthesize.rs:114-132
        n = self.domain().size
        return [[self.values[row[0][col]] for row in self.rows] + [0] * (n - len(self.rows)) for col in range(WIRES)]


def arithmetic_rows(sel, w, pi, r):
    """the gate equation of every row (composer/mod.rs test `compose`)"""
    return [(sel["q_0"][i] * w[0][i] + sel["q_1"][i] * w[1][i] + sel["q_2"][i] * w[2][i] + sel["q_3"][i] * w[3][i]
             + sel["q_m"][i] * w[1][i] * w[2][i] + sel["q_c"][i] + pi[i]) % r for i in range(sel["n"])]


def inv0(x, r):
    """1 / x with the library's convention for the case where the reference panics: 1 / 0 = 0"""
    return pow(x, -1, r) if x % r else 0


def perm_terms(w, sigma, roots, ks, beta, gamma, r):
    """perm[i] of compute_z (indexer/permutation.rs:88-103)"""
    out = []
    for i in range(len(roots)):
        num = den = 1
        for j in range(WIRES):
            num = num * (w[j][i] + ks[j] * beta * roots[i] + gamma) % r
            den = den * (w[j][i] + beta * sigma[j][i] + gamma) % r
        out.append(num * inv0(den, r) % r)
    return out


def prefix_product(v, r):
    """(exclusive running product, total)"""
    out, acc = [], 1
    for x in v:
        out.append(acc)
        acc = acc * x % r
    return out, acc


def compute_z(w, sigma, roots, ks, beta, gamma, r):
    """(z over domain_n, closes): permutation.rs:105-112"""
    z, total = prefix_product(perm_terms(w, sigma, roots, ks, beta, gamma, r), r)
    return z, total == 1


def coset_points(curve, log_n):
    """linear_4n (permutation.rs:134-137): x_i = g w^i over domain_4n"""
    c = CURVES[curve] if not hasattr(curve, "r") else curve
    d = Domain(c, 4 << log_n)
    out, x = [], d.coset_gen
    for _ in range(d.size):
        out.append(x)
        x = x * d.group_gen % c.r
    return out


def v_4n_inversed(curve, log_n):
    """indexer/mod.rs:223-225: the coset_fft of X^n - 1 over domain_4n, inverted point by point"""
    c = CURVES[curve] if not hasattr(curve, "r") else curve
    n = 1 << log_n
    v_poly = [c.r - 1] + [0] * (n - 1) + [1]
    return [pow(v, -1, c.r) for v in Domain(c, 4 * n).coset_fft(v_poly)]


def v_4n_inversed_four(curve, log_n):
    """the same from four values: x_i^n = g^n (w^n)^(i mod 4)"""
    c = CURVES[curve] if not hasattr(curve, "r") else curve
    n = 1 << log_n
    d = Domain(c, 4 * n)
    gn, iota = pow(d.coset_gen, n, c.r), pow(d.group_gen, n, c.r)
    four = [pow(gn * pow(iota, k, c.r) - 1, -1, c.r) for k in range(4)]
    return [four[i % 4] for i in range(4 * n)]


def quotient_pointwise(t, xs, vinv, ks, beta, gamma, alpha, r):
    """prover.rs:184-202 over tables t[name] of N values: arithmetic.rs:90-116, permutation.rs:148-167, then * v_4n_inversed"""
    N = len(xs)
    out = []
    for i in range(N):
        w = [t[f"w_{j}"][i] for j in range(WIRES)]
        if t["q_arith"][i] == 0:
            arith = 0
        else:
            arith = (t["q_0"][i] * w[0] + t["q_1"][i] * w[1] + t["q_2"][i] * w[2] + t["q_3"][i] * w[3] + t["q_m"][i] * w[1] * w[2]
                     + t["q_c"][i] + t["pi"][i]) * t["q_arith"][i] % r
        nxt = i % 4 if i // 4 == N // 4 - 1 else i + 4
        num, den = t["z"][i], t["z"][nxt]
        for j in range(WIRES):
            num = num * (w[j] + ks[j] * beta * xs[i] + gamma) % r
            den = den * (w[j] + beta * t[f"sigma_{j}"][i] + gamma) % r
        perm = ((num - den) * alpha + (t["z"][i] - 1) * t["l1"][i] * alpha * alpha) % r
        out.append((arith + perm) * vinv[i] % r)
    return out


class RefIndex:
    """AHPForPLONK::index (indexer/mod.rs:128-256)"""

    def __init__(self, cs, ks):
        self.curve, self.r, self.ks = cs.curve, cs.r, [k % cs.r for k in ks]
        self.sel = cs.compose(self.ks)
        self.n = self.sel["n"]
        self.log_n = self.n.bit_length() - 1
        self.dn, self.d4 = Domain(self.curve, self.n), Domain(self.curve, 4 * self.n)
        self.roots = cs.roots()
        self.on_4n = {name: self.extend(self.sel[name]) for name in Q_NAMES + S_NAMES}
        self.on_4n["l1"] = self.extend([1] + [0] * (self.n - 1))
        self.vinv = v_4n_inversed(self.curve, self.log_n)
        self.xs = coset_points(self.curve, self.log_n)

    def extend(self, evals):
        return self.d4.coset_fft(self.dn.ifft(evals))


def prove_rounds(ix, witnesses, public_inputs, beta, gamma, alpha):
    """prover_init and rounds 1-3: dict of coefficient vectors w_0..w_3, z, t_0..t_3 (n each) plus `closes`"""
    r, n = ix.r, ix.n
    out = {}
    t = dict(ix.on_4n)
    t["pi"] = ix.extend(list(public_inputs) + [0] * (n - len(public_inputs)))
    for j in range(WIRES):
        out[f"w_{j}"] = ix.dn.ifft(witnesses[j])
        t[f"w_{j}"] = ix.d4.coset_fft(out[f"w_{j}"])
    z, out["closes"] = compute_z(witnesses, [ix.sel[s] for s in S_NAMES], ix.roots, ix.ks, beta, gamma, r)
    out["z_evals"] = z
    out["z"] = ix.dn.ifft(z)
    t["z"] = ix.d4.coset_fft(out["z"])
    tq = ix.d4.coset_ifft(quotient_pointwise(t, ix.xs, ix.vinv, ix.ks, beta, gamma, alpha, r))
    for k in range(4):
        out[f"t_{k}"] = tq[k * n:(k + 1) * n]
    return out


def horner(coeffs, x, r):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % r
    return acc


def round3_identity(ix, polys, public_inputs, beta, gamma, alpha, zeta):
    """(t(zeta) (zeta^n - 1), arith(zeta) + perm(zeta)) with every polynomial evaluated from its coefficient vector:
    t = t_0 + zeta^n t_1 + zeta^2n t_2 + zeta^3n t_3; z(w zeta) is z shifted one row."""
    r, n = ix.r, ix.n
    ev = lambda evals: horner(ix.dn.ifft(evals), zeta, r)              # noqa: E731
    zn = pow(zeta, n, r)
    t = sum(horner(polys[f"t_{k}"], zeta, r) * pow(zn, k, r) for k in range(4)) % r
    w = [horner(polys[f"w_{j}"], zeta, r) for j in range(WIRES)]
    q = {name: ev(ix.sel[name]) for name in Q_NAMES + S_NAMES}
    pi = ev(list(public_inputs) + [0] * (n - len(public_inputs)))
    arith = (q["q_0"] * w[0] + q["q_1"] * w[1] + q["q_2"] * w[2] + q["q_3"] * w[3] + q["q_m"] * w[1] * w[2] + q["q_c"] + pi) * q["q_arith"] % r
    z, z_next = horner(polys["z"], zeta, r), horner(polys["z"], zeta * ix.dn.group_gen % r, r)
    num, den = z, z_next
    for j in range(WIRES):
        num = num * (w[j] + ix.ks[j] * beta * zeta + gamma) % r
        den = den * (w[j] + beta * q[f"sigma_{j}"] + gamma) % r
    l1 = (zn - 1) * pow(n * (zeta - 1), -1, r) % r                     # evaluate_first_lagrange_poly (utils.rs:45-50)
    perm = ((num - den) * alpha + (z - 1) * l1 * alpha * alpha) % r
    return t * (zn - 1) % r, (arith + perm) % r
