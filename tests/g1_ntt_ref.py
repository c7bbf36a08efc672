"""Python-integer references for the transforms over G1 (zkp_g1_scale_vec_dev / zkp_g1_ntt_dev) and for asvc.prove_all.

Inputs of the device tests are P_j = [a_j] G with known exponents a_j, so every expected point is [e] G for an exponent e that
oracle/pyref computes in Fr (Domain.fft / ifft for the transform): n scalar multiplications instead of n^2.  `FixedBase` makes those
multiplications cheap: the multiples d 2^(8 k) G of oracle/pyref/curves.Group's additions, built once per curve, then 32 additions
and one inversion per exponent, cached by exponent.  Points are (x, y) or None, as in oracle/pyref."""
from __future__ import annotations

import numpy as np

from ckb_zkp_amd import codec
from ckb_zkp_amd.params import get_curve
from oracle.pyref.curves import Group
from oracle.pyref.fields import CURVES
from oracle.pyref.ntt import Domain

WINDOW = 8


class FixedBase:
    """[k] G for the curve's G1 generator"""
    _made: dict = {}

    def __new__(cls, curve: str):
        if curve not in cls._made:
            self = super().__new__(cls)
            self.c = CURVES[curve]
            self.g = Group(self.c, 1)
            self.rows = []
            base = self.g.to_jac(self.c.g1_gen)
            for _ in range((self.c.r.bit_length() + WINDOW - 1) // WINDOW):
                row, acc = [None], None
                for _d in range(1, 1 << WINDOW):
                    acc = base if acc is None else self.g.jadd(acc, base)
                    row.append(acc)
                self.rows.append(row)
                for _b in range(WINDOW):
                    base = self.g.jdbl(base)
            self.cache = {0: None}
            cls._made[curve] = self
        return cls._made[curve]

    def mul(self, k: int):
        k %= self.c.r
        if k not in self.cache:
            acc, e, i = None, k, 0
            while e:
                d = e & ((1 << WINDOW) - 1)
                if d:
                    acc = self.rows[i][d] if acc is None else self.g.jadd(acc, self.rows[i][d])
                e >>= WINDOW
                i += 1
            self.cache[k] = self.g.to_affine(acc)
        return self.cache[k]


def points(curve: str, exps):
    """[e] G for every exponent -> ((n, w) affine Montgomery words, (n,) identity flags) as the device writes them"""
    fb = FixedBase(curve)
    return codec.g1_to_mont([fb.mul(e) for e in exps], get_curve(curve))


def fr_transform(curve: str, a, inverse: bool):
    """out[i] = sum_j w^(i j) a_j, or (1/n) sum_j w^(-i j) a_j, over the domain of zkp_ntt_dev"""
    d = Domain(CURVES[curve], len(a))
    assert d.size == len(a)
    return d.ifft(list(a)) if inverse else d.fft(list(a))


def prove_all_exponents(curve: str, n: int, tau: int, values):
    """the arrangement of asvc.prove_all with every point replaced by its exponent: the n values q_i(tau)"""
    c = CURVES[curve]
    r = c.r
    small, big = Domain(c, n), Domain(c, 2 * n)
    assert small.size == n and big.size == 2 * n
    a = [pow(tau, n - 2 - k, r) for k in range(n - 1)] + [0] * (n + 1)
    coeffs = small.ifft(list(values) + [0] * (n - len(values)))
    big_a, big_b = big.fft(a), big.fft(coeffs + [0] * n)
    conv = big.ifft([x * y % r for x, y in zip(big_a, big_b)])
    return small.fft(conv[n - 1:2 * n - 1])
