"""Bulletproofs for R1CS in Python integers and oracle.pyref curve arithmetic: the prover (bulletproofs/src/arithmetic_circuit.rs:
305-612, inner_product_proof.rs:22-111) and the verifier (:614-848, inner_product_proof.rs:113-174), written from the protocol's
equations.  The prover takes the inputs and callbacks of ckb_zkp_amd.bulletproofs.prove and returns the same Proof, so the two are
compared field for field; inside, field elements are integers and points are affine (x, y) tuples or None.

With f = inputs ++ aux, the rows A_i, B_i, C_i of the system, k inputs and the witness columns k ..:
  aL = A f, aR = B f, aO = C f;   Y_i = y^i, Z_i = z^(i+1) (i < n), zn = z^n, U_i = zn Z_i / Y_i
  v_j = sum_i Z_i (A + zn B + zn^2 C)[i][k + j]
  l(X) = (aL + U) X^2 + aO X^3 + w X^4 + sL X^5,   r(X) = -v + (zn^2 Z - Y) X + (Y aR + Z) X^2 + Y sR X^5
  t(X) = <l(X), r(X)> = sum_d t_d X^d, d = 2 .. 10; t_4 is not committed: the verifier knows it."""
import numpy as np

from ckb_zkp_amd import codec
from ckb_zkp_amd.bulletproofs import T_DEGREES, Proof, drawer
from ckb_zkp_amd.r1cs import INPUT
from oracle.pyref.curves import Group
from oracle.pyref.fields import CURVES as OC

L_DEGREES, R_DEGREES = (2, 3, 4, 5), (0, 1, 2, 5)


def group(c):
    return Group(OC[c.name], 1)


def msm(G, pairs):
    """sum of k P over (k, P) pairs -> affine: double-and-add with the doublings shared by all terms"""
    terms = [(k % G.order, p) for k, p in pairs if p is not None and k % G.order]
    acc = G.to_jac(None)
    for bit in range(max((k.bit_length() for k, _ in terms), default=0) - 1, -1, -1):
        acc = G.jdbl(acc)
        for k, p in terms:
            if (k >> bit) & 1:
                acc = G.jadd_mixed(acc, p)
    return G.to_affine(acc)


def abi_point(P, c):
    xy, inf = codec.g1_to_mont([P], c)
    return xy[0], bool(inf[0])


def int_point(pt, c):
    return codec.g1_from_mont(np.asarray(pt[0], dtype=np.uint64).reshape(1, -1), [pt[1]], c)[0]


def dense_rows(cs, which):
    """rows of one constraint matrix as {column: coefficient}; columns index inputs ++ aux"""
    out = []
    for row in {"a": cs.at, "b": cs.bt, "c": cs.ct}[which]:
        d = {}
        for coeff, (kind, j) in row:
            col = j if kind == INPUT else cs.num_inputs + j
            d[col] = (d.get(col, 0) + coeff) % cs.curve.r
        out.append(d)
    return out


def dot(a, b, r):
    return sum(x * y for x, y in zip(a, b)) % r


def _yz_vectors(y, z, n, N, r):
    """Y_i = y^i, Z_i = z^(i+1) below n and 0 from n on, zn = z^n, U_i = zn Z_i / Y_i"""
    yi, zn = pow(y, -1, r), pow(z, n, r)
    Y, Z, U = [], [], []
    yp, zp, up, q = 1, z, zn * z % r, z * yi % r
    for i in range(N):
        Y.append(yp)
        Z.append(zp if i < n else 0)
        U.append(up if i < n else 0)
        yp, zp, up = yp * y % r, zp * z % r, up * q % r
    return Y, Z, zn, U


def _combined(cs, zn, r):
    """W = A + zn B + zn^2 C as rows of {column: coefficient}"""
    a, b, cc = dense_rows(cs, "a"), dense_rows(cs, "b"), dense_rows(cs, "c")
    rows = []
    for ra, rb, rc in zip(a, b, cc):
        d = {}
        for src, k in ((ra, 1), (rb, zn), (rc, zn * zn % r)):
            for col, v in src.items():
                d[col] = (d.get(col, 0) + k * v) % r
        rows.append(d)
    return rows


def lr_from_vectors(a_l, a_r, a_o, w, v, s_l, s_r, N, y, z, r):
    """({degree: vector} of l, {degree: vector} of r), N elements each, from vectors without their zero padding"""
    n = len(a_l)
    assert len(a_r) == len(a_o) == n and len(w) == len(v) and len(s_l) == len(s_r) and max(n, len(w), len(s_l)) <= N
    pad = lambda vec: list(vec) + [0] * (N - len(vec))            # noqa: E731
    a_l, a_r, a_o, w, v, s_l, s_r = (pad(t) for t in (a_l, a_r, a_o, w, v, s_l, s_r))
    Y, Z, zn, U = _yz_vectors(y, z, n, N, r)
    zn2 = zn * zn % r
    lp = {2: [(a_l[i] + U[i]) % r for i in range(N)], 3: a_o, 4: w, 5: s_l}
    rp = {0: [-e % r for e in v], 1: [(zn2 * Z[i] - Y[i]) % r for i in range(N)],
          2: [(Y[i] * a_r[i] + Z[i]) % r for i in range(N)], 5: [Y[i] * s_r[i] % r for i in range(N)]}
    return lp, rp


def lr_polys(cs, s_l, s_r, y, z):
    """the same from a constraint system with its assignment and the blinding vectors"""
    r = cs.curve.r
    n, k, n_w = cs.num_constraints(), cs.num_inputs, cs.num_aux
    N = 1 << (max(n, n_w) - 1).bit_length()
    f = cs.full_assignment()
    a_l, a_r, a_o = ([sum(v * f[col] for col, v in row.items()) % r for row in dense_rows(cs, m)] for m in "abc")
    Z = [pow(z, i + 1, r) for i in range(n)]
    v = [0] * n_w
    for i, row in enumerate(_combined(cs, pow(z, n, r), r)):
        for col, val in row.items():
            if col >= k:
                v[col - k] = (v[col - k] + Z[i] * val) % r
    return lr_from_vectors(a_l, a_r, a_o, f[k:], v, s_l, s_r, N, y, z, r)


def t_coeffs(lp, rp, r):
    """{d: t_d} for d = 2 .. 10: the convolution of the two coefficient lists"""
    t = {d: 0 for d in range(2, 11)}
    for a in L_DEGREES:
        for b in R_DEGREES:
            t[a + b] = (t[a + b] + dot(lp[a], rp[b], r)) % r
    return t


def eval_vec_poly(p, x, r):
    N = len(next(iter(p.values())))
    xs = {d: pow(x, d, r) for d in p}
    return [sum(vec[i] * xs[d] for d, vec in p.items()) % r for i in range(N)]


def prove(curve, cs, gens, rand, challenger) -> Proof:
    """gens: (g_vec, h_vec, g, h, u) as integer points"""
    c = cs.curve
    r = c.r
    G = group(c)
    g_vec, h_vec, g, h, u = gens
    n, k, n_w = cs.num_constraints(), cs.num_inputs, cs.num_aux
    n_max = max(n, n_w)
    N = 1 << (n_max - 1).bit_length()
    assert len(g_vec) == len(h_vec) == N
    f = cs.full_assignment()
    draw = drawer(rand, 2 * n_max + 12)
    s_l, s_r = draw(n_max), draw(n_max)
    bl_i, bl_o, bl_s, bl_w = draw(4)
    a_l, a_r, a_o = ([sum(v * f[col] for col, v in row.items()) % r for row in dense_rows(cs, m)] for m in "abc")
    a_i = msm(G, [(bl_i, h)] + list(zip(a_l, g_vec)) + list(zip(a_r, h_vec)))
    a_out = msm(G, [(bl_o, h)] + list(zip(a_o, g_vec)))
    a_w = msm(G, [(bl_w, h)] + list(zip(f[k:], g_vec)))
    s_pt = msm(G, [(bl_s, h)] + list(zip(s_l, g_vec)) + list(zip(s_r, h_vec)))
    y, z = (int(t) % r for t in challenger.yz(*(abi_point(p, c) for p in (a_i, a_out, a_w, s_pt))))
    lp, rp = lr_polys(cs, s_l, s_r, y, z)
    t = t_coeffs(lp, rp, r)
    taus = draw(8)
    t_pts = [msm(G, [(t[d], g), (tau, h)]) for d, tau in zip(T_DEGREES, taus)]
    x = int(challenger.x([abi_point(p, c) for p in t_pts])) % r
    l_x, r_x = eval_vec_poly(lp, x, r), eval_vec_poly(rp, x, r)
    t_x = dot(l_x, r_x, r)
    tau_x = sum(tau * pow(x, d, r) for d, tau in zip(T_DEGREES, taus)) % r
    mu = (bl_i * x ** 2 + bl_o * x ** 3 + bl_w * x ** 4 + bl_s * x ** 5) % r
    lx_abi, rx_abi = codec.fr_to_mont(l_x, c), codec.fr_to_mont(r_x, c)
    x_1 = int(challenger.x1(t_x, tau_x, mu, lx_abi, rx_abi)) % r
    ux = G.mul(u, x_1)
    ipp_p = msm(G, list(zip(l_x, g_vec)) + list(zip(r_x, h_vec)) + [(t_x, ux)])
    proof = Proof(abi_point(a_i, c), abi_point(a_out, c), abi_point(a_w, c), abi_point(s_pt, c), [abi_point(p, c) for p in t_pts],
                  mu, tau_x, lx_abi, rx_abi, t_x, abi_point(ipp_p, c))
    a, b, gv, hv = list(l_x), list(r_x), list(g_vec), list(h_vec)
    while len(a) > 1:
        m = len(a) // 2
        c_l, c_r = dot(a[:m], b[m:], r), dot(a[m:], b[:m], r)
        l_pt = msm(G, list(zip(a[:m], gv[m:])) + list(zip(b[m:], hv[:m])) + [(c_l, ux)])
        r_pt = msm(G, list(zip(a[m:], gv[:m])) + list(zip(b[:m], hv[m:])) + [(c_r, ux)])
        l_abi, r_abi = abi_point(l_pt, c), abi_point(r_pt, c)
        proof.L_vec.append(l_abi)
        proof.R_vec.append(r_abi)
        e = int(challenger.ipa(l_abi, r_abi)) % r
        ei = pow(e, -1, r)
        gv = [msm(G, [(ei, gv[j]), (e, gv[j + m])]) for j in range(m)]
        hv = [msm(G, [(e, hv[j]), (ei, hv[j + m])]) for j in range(m)]
        a = [(e * a[j] + ei * a[j + m]) % r for j in range(m)]
        b = [(ei * b[j] + e * b[j + m]) % r for j in range(m)]
    proof.a, proof.b = a[0], b[0]
    return proof


def verify(curve, cs, gens, proof: Proof, public_inputs, challenger) -> bool:
    """cs supplies the matrices and shape only; public_inputs are the inputs after the leading one.  Three checks: the
    inner-product argument for IPP_P, the commitment to t(x), and P against l_x, r_x."""
    c = cs.curve
    r = c.r
    G = group(c)
    g_vec, h_vec, g, h, u = gens
    n, k, n_w = cs.num_constraints(), cs.num_inputs, cs.num_aux
    N = len(g_vec)
    s = [1] + [int(v) % r for v in public_inputs]
    if len(s) != k or proof.l_x.shape != (N, 4) or proof.r_x.shape != (N, 4):
        return False
    rounds = N.bit_length() - 1
    if len(proof.L_vec) != rounds or len(proof.R_vec) != rounds or len(proof.T) != len(T_DEGREES):
        return False
    pt = lambda p: int_point(p, c)                                # noqa: E731
    y, z = (int(t) % r for t in challenger.yz(proof.A_I, proof.A_O, proof.A_W, proof.S))
    x = int(challenger.x(list(proof.T))) % r
    x_1 = int(challenger.x1(proof.t_x, proof.tau_x, proof.mu, proof.l_x, proof.r_x)) % r
    ux = G.mul(u, x_1)
    l_x, r_x = codec.fr_from_mont(proof.l_x, c), codec.fr_from_mont(proof.r_x, c)
    # ---- the inner-product argument: a g' + b h' + a b ux == P + sum x_j^2 L_j + x_j^-2 R_j
    es = [int(challenger.ipa(l, rr)) % r for l, rr in zip(proof.L_vec, proof.R_vec)]
    if any(e == 0 for e in es):
        return False
    eis = [pow(e, -1, r) for e in es]
    sv = []
    for i in range(N):
        acc = 1
        for j in range(rounds):                                   # round j halves on index bit rounds - 1 - j
            acc = acc * (es[j] if (i >> (rounds - 1 - j)) & 1 else eis[j]) % r
        sv.append(acc)
    terms = [(proof.a * sv[i], g_vec[i]) for i in range(N)] + [(proof.b * pow(sv[i], -1, r), h_vec[i]) for i in range(N)]
    terms += [(proof.a * proof.b, ux), (-1, pt(proof.IPP_P))]
    terms += [(-e * e, pt(l)) for e, l in zip(es, proof.L_vec)] + [(-ei * ei, pt(rr)) for ei, rr in zip(eis, proof.R_vec)]
    if msm(G, terms) is not None:
        return False
    # ---- t_x g + tau_x h == x^4 (delta + <z_Q, c>) g + sum_d x^d T_d
    Y, Z, zn, U = _yz_vectors(y, z, n, N, r)
    comb = _combined(cs, zn, r)
    delta = dot(U, Z, r)
    zq_c = sum(Z[i] * sum(val * s[col] for col, val in row.items() if col < k) for i, row in enumerate(comb)) % r
    terms = [(proof.t_x - pow(x, 4, r) * (delta + zq_c), g), (proof.tau_x, h)]
    terms += [(-pow(x, d, r), pt(t)) for d, t in zip(T_DEGREES, proof.T)]
    if msm(G, terms) is not None:
        return False
    # ---- x^2 A_I + x^3 A_O + x^4 A_W + x^5 S + sum_i (x^2 U_i) g_i + (x (zn^2 Z_i - Y_i) + x^2 Z_i - v_i) h'_i
    #      == mu h + <l_x, g> + <r_x, h'>,   h'_i = y^-i h_i
    v = [0] * N
    for i, row in enumerate(comb):
        for col, val in row.items():
            if col >= k:
                v[col - k] = (v[col - k] + Z[i] * val) % r
    yi = pow(y, -1, r)
    x2 = x * x % r
    terms = [(x2, pt(proof.A_I)), (x2 * x, pt(proof.A_O)), (x2 * x2, pt(proof.A_W)), (x2 * x2 * x, pt(proof.S)), (-proof.mu, h)]
    for i in range(N):
        terms.append((x2 * U[i] - l_x[i], g_vec[i]))
        terms.append(((x * (zn * zn * Z[i] - Y[i]) + x2 * Z[i] - v[i] - r_x[i]) * pow(yi, i, r), h_vec[i]))
    return msm(G, terms) is None
