"""The matrix polynomial commitments of hyrax, libra and spartan in Python integers over oracle.pyref.curves: poly_commit_vec,
packing_poly_commit (spartan/src/commitments.rs:10-56), BulletReduceProof prover / verify, LogDotProductProof prover / verify and
reduce_prover / reduce_verifier (hyrax/src/commitment.rs:335-625), written from the protocol's equations.  The provers take the
inputs and callbacks of ckb_zkp_amd.polycommit and return the same values, so the two are compared field for field; inside, field
elements are integers and points are affine (x, y) tuples or None.

Parity with the Rust reference is unpinned: it cannot be built here, and its challenges come from a merlin transcript that stays
with the caller.  HashChallenger below stands in for it in the tests, shared by prover and verifier."""
import hashlib

import numpy as np

from ckb_zkp_amd import codec
from ckb_zkp_amd.bulletproofs import drawer
from ckb_zkp_amd.polycommit import split_sizes
from tests.bulletproofs_ref import abi_point, group, int_point, msm


class RefParams:
    """gen_n: n generators and h; gen_1: g1 and the same h"""

    def __init__(self, curve, gens, h, g1):
        self.c, self.G, self.gens, self.h, self.g1, self.n = curve, group(curve), list(gens), h, g1, len(gens)

    @classmethod
    def of(cls, params):
        """the integer view of a ckb_zkp_amd.polycommit.Params"""
        c = params.curve
        return cls(c, codec.g1_from_mont(params.gens_xy, params.gens_inf, c), int_point((params.h_xy, False), c),
                   int_point((params.g1_xy, False), c))


class HashChallenger:
    """append(label, point) / challenge(label) -> non-zero integer below r: SHA-256 over everything seen so far.  Points may be
    integer tuples, None, or (xy, inf) device-format points: both forms of one point hash alike."""

    def __init__(self, curve, seed=b""):
        self.c, self.state, self.log = curve, hashlib.sha256(b"polycommit" + seed).digest(), []

    def append(self, label, point):
        if point is not None and isinstance(point[0], np.ndarray):
            point = int_point(point, self.c)
        data = b"inf" if point is None else point[0].to_bytes(48, "little") + point[1].to_bytes(48, "little")
        self.state = hashlib.sha256(self.state + label.encode() + b":" + data).digest()
        self.log.append(label)

    def challenge(self, label):
        self.state = hashlib.sha256(self.state + b"challenge " + label.encode()).digest()
        self.log.append(label)
        return int.from_bytes(self.state[:31], "little") % self.c.r or 1


def log2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


def dot(a, b, r):
    return sum(x * y for x, y in zip(a, b)) % r


def eval_eq(rs, r):
    """out[idx] = prod_i (bit_{k-1-i}(idx) ? rs[i] : 1 - rs[i]): rs[0] decides the most significant bit"""
    out = [1]
    for x in rs:
        out = [v * f % r for v in out for f in ((1 - x) % r, x % r)]
    return out


def poly_commit_vec(P, gens, values, h, blind):
    return msm(P.G, [(v, g) for v, g in zip(values, gens)] + [(blind, h)])


def packing_poly_commit(P, values, rand, is_blind):
    l_size, r_size = split_sizes(log2(len(values)))
    blinds = [b % P.c.r for b in drawer(rand, l_size)(l_size)] if is_blind else [0] * l_size
    return [poly_commit_vec(P, P.gens, values[i * r_size:(i + 1) * r_size], P.h, blinds[i]) for i in range(l_size)], blinds


def bullet_reduce_prove(P, a_vec, b_vec, blind_gamma, blind_vec, ch):
    r, G = P.c.r, P.G
    a, b, g = list(a_vec), list(b_vec), list(P.gens[:len(a_vec)])
    n = len(a)
    assert len(b) == n and n & (n - 1) == 0
    l_vec, r_vec, blind_fin = [], [], blind_gamma % r
    for blind_l, blind_r in blind_vec[:log2(n)]:
        n //= 2
        al, ar, bl, br, gl, gr = a[:n], a[n:], b[:n], b[n:], g[:n], g[n:]
        cl, cr = dot(al, br, r), dot(ar, bl, r)
        l_pt = msm(G, list(zip(al, gr)) + [(cl, P.g1), (blind_l, P.h)])
        r_pt = msm(G, list(zip(ar, gl)) + [(cr, P.g1), (blind_r, P.h)])
        l_vec.append(l_pt)
        r_vec.append(r_pt)
        ch.append("L", l_pt)
        ch.append("R", r_pt)
        x = ch.challenge("x") % r
        xi = pow(x, -1, r)
        g = [msm(G, [(xi, gl[i]), (x, gr[i])]) for i in range(n)]
        a = [(al[i] * x + ar[i] * xi) % r for i in range(n)]
        b = [(bl[i] * xi + br[i] * x) % r for i in range(n)]
        blind_fin = (blind_fin + x * x * blind_l + xi * xi * blind_r) % r
    gamma_hat = msm(G, [(a[0], g[0]), (a[0] * b[0], P.g1), (blind_fin, P.h)])
    return (l_vec, r_vec), gamma_hat, a[0], b[0], g[0], blind_fin


def bullet_reduce_verify(P, l_vec, r_vec, g_vec, gamma, b_vec, ch):
    r, G = P.c.r, P.G
    lg_n = len(l_vec)
    n = 1 << lg_n
    assert len(r_vec) == lg_n and len(b_vec) == n and len(g_vec) >= n
    x_sq, x_inv_sq, allinv = [], [], 1
    for l_pt, r_pt in zip(l_vec, r_vec):
        ch.append("L", l_pt)
        ch.append("R", r_pt)
        x = ch.challenge("x") % r
        xi = pow(x, -1, r)
        x_sq.append(x * x % r)
        x_inv_sq.append(xi * xi % r)
        allinv = allinv * xi % r
    s = [allinv]
    for i in range(1, n):
        lg_i = i.bit_length() - 1
        s.append(s[i - (1 << lg_i)] * x_sq[lg_n - 1 - lg_i] % r)
    b_s = dot(b_vec, s, r)
    g_hat = msm(G, list(zip(s, g_vec)))
    gamma_hat = msm(G, list(zip(x_sq, l_vec)) + list(zip(x_inv_sq, r_vec)) + [(1, gamma)])
    return b_s, g_hat, gamma_hat


def log_dot_product_prove(P, x_vec, blind_x, a_vec, y, blind_y, rand, ch):
    """-> (proof, comm_x, comm_y), proof = (l_vec, r_vec, delta, beta, z1, z2), points as integer tuples"""
    r = P.c.r
    size = len(a_vec)
    assert len(x_vec) == size and P.n >= size
    k = log2(size)
    draw = drawer(rand, 3 + 2 * k)
    d, r_beta, r_delta = (v % r for v in draw(3))
    blind_vec = [tuple(v % r for v in draw(2)) for _ in range(k)]
    comm_x = poly_commit_vec(P, P.gens, x_vec, P.h, blind_x)
    ch.append("Cx", comm_x)
    comm_y = poly_commit_vec(P, [P.g1], [y], P.h, blind_y)
    ch.append("Cy", comm_y)
    (l_vec, r_vec), _gamma_hat, x_hat, a_hat, g_hat, r_hat_gamma = bullet_reduce_prove(P, x_vec, a_vec, blind_x + blind_y, blind_vec, ch)
    y_hat = x_hat * a_hat % r
    delta = poly_commit_vec(P, [g_hat], [d], P.h, r_delta)
    ch.append("delta", delta)
    beta = poly_commit_vec(P, [P.g1], [d], P.h, r_beta)
    ch.append("beta", beta)
    c = ch.challenge("c") % r
    z1 = (d + c * y_hat) % r
    z2 = (a_hat * (c * r_hat_gamma + r_beta) + r_delta) % r
    return (l_vec, r_vec, delta, beta, z1, z2), comm_x, comm_y


def log_dot_product_verify(P, proof, comm_x, comm_y, a_vec, ch):
    l_vec, r_vec, delta, beta, z1, z2 = proof
    G, r = P.G, P.c.r
    ch.append("Cx", comm_x)
    ch.append("Cy", comm_y)
    gamma = G.add(comm_x, comm_y)
    a_hat, g_hat, gamma_hat = bullet_reduce_verify(P, l_vec, r_vec, P.gens, gamma, a_vec, ch)
    ch.append("delta", delta)
    ch.append("beta", beta)
    c = ch.challenge("c") % r
    lhs = G.add(G.mul(G.add(G.mul(gamma_hat, c), beta), a_hat), delta)
    rhs = G.add(G.mul(G.add(g_hat, G.mul(P.g1, a_hat)), z1 % r), G.mul(P.h, z2 % r))
    return lhs == rhs


def row_fold(poly, ry, r):
    """(lz, L, R): lz[j] = sum_i L[i] poly[i r_size + j] with the two eq tables of ry"""
    size = log2(len(poly))
    l_size, r_size = split_sizes(size)
    l_eq, r_eq = eval_eq(ry[:size // 2], r), eval_eq(ry[size // 2:], r)
    return [sum(l_eq[i] * poly[i * r_size + j] for i in range(l_size)) % r for j in range(r_size)], l_eq, r_eq


def reduce_prover(P, poly, blind_poly, ry, ry_blind, eval_, rand, ch):
    """-> (proof, comm_y)"""
    r = P.c.r
    assert len(ry) == log2(len(poly))
    lz, l_eq, r_eq = row_fold(poly, ry, r)
    blinds = list(blind_poly) if len(blind_poly) else [0] * len(l_eq)
    assert len(blinds) == len(l_eq)
    proof, _, comm_y = log_dot_product_prove(P, lz, dot(l_eq, blinds, r), r_eq, eval_, ry_blind, rand, ch)
    return proof, comm_y


def reduce_verifier(P, proof, ry, comms_witness, comm_ry, ch):
    size = len(ry)
    r = P.c.r
    l_eq, r_eq = eval_eq(ry[:size // 2], r), eval_eq(ry[size // 2:], r)
    comm_lz = msm(P.G, list(zip(l_eq, comms_witness)))
    return log_dot_product_verify(P, proof, comm_lz, comm_ry, r_eq, ch)


def proof_to_abi(proof, c):
    l_vec, r_vec, delta, beta, z1, z2 = proof
    return [abi_point(p, c) for p in l_vec], [abi_point(p, c) for p in r_vec], abi_point(delta, c), abi_point(beta, c), z1, z2


def proof_to_int(proof, c):
    l_vec, r_vec, delta, beta, z1, z2 = proof
    return [int_point(p, c) for p in l_vec], [int_point(p, c) for p in r_vec], int_point(delta, c), int_point(beta, c), z1, z2


def same_point(a, b):
    return bool(a[1]) == bool(b[1]) and np.array_equal(np.asarray(a[0]), np.asarray(b[0]))


def same_proof(a, b):
    """two device-format proofs, bit for bit"""
    return (len(a[0]) == len(b[0]) and len(a[1]) == len(b[1]) and all(same_point(p, q) for p, q in zip(a[0], b[0])) and
            all(same_point(p, q) for p, q in zip(a[1], b[1])) and same_point(a[2], b[2]) and same_point(a[3], b[3]) and
            a[4] == b[4] and a[5] == b[5])
