// The tower above Fq2 and the optimal-ate pairing on it, for BN254 and BLS12-381: Fq6 = Fq2[v] / (v^3 - xi), Fq12 = Fq6[w] / (w^2 - v),
// the Miller loop on the twist and the final exponentiation.  Replaces ark-ec's `miller_loop` / `final_exponentiation` that the reference
// reaches from groth16/src/verifier.rs:8-44 and marlin/src/pc/kzg10.rs:158-173.
//
// Everything is a template over C (the curve's struct of pairing_constants.inc) and F2 (an Fq2 with members c0, c1 of type F2::B, the
// operators + - *, sqr, dbl, neg, inv, zero, one): the device instantiates it with Fp2<P> of field_dev.hpp, tests/c/pairing_host.cpp
// with a plain C++ field, so the formulas are checked on a CPU, word for word, before a device runs them.  Plain C++ over the field's
// operators: no assembly here.
//
// Layout: an Fq12 is c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (ark's order, the ABI's); c_j.c_i is the coefficient of w^(2 i + j).
//
// Code size: the Montgomery product is one out-of-line copy per field (this unit is built WITHOUT ZKP_INLINE_MUL) and every Fq6 / Fq12
// routine below is out of line too; an Fq12 (96 / 144 words) does not live in registers across them, it lives in the lane's private
// memory and the routines work on one Fq2 coefficient at a time.
//
// Miller loop: T on the twist in homogeneous projective coordinates, doubling and mixed addition with inversion-free lines (Costello,
// Lange, Naehrig, "Faster pairing computations on curves with high-degree twists"; the formulas as ark-ec 0.2 models/bn/g2.rs states
// them).  A line is A + B w with A = a0 + a1 v, B = b0 + b1 v: D-type (BN254) a1 = 0, M-type (BLS12-381) b0 = 0; lines are scaled by
// Fq2 factors that the final exponentiation removes.  BN254 walks the bits of 6x + 2 and adds the Frobenius images Q1, -Q2;
// BLS12-381 walks |x| and conjugates, x being negative.
//
// Final exponentiation: f^((q^6 - 1)(q^2 + 1)) with one inversion, then the hard part as a polynomial in q evaluated with Frobenius
// maps, powers by x and Granger-Scott squarings ("Faster squaring in the cyclotomic subgroup of sixth degree extensions"):
//   BN254     (q^4 - q^2 + 1) / r = q^3 + (6x^2 + 1) q^2 + (-36x^3 - 18x^2 - 12x + 1) q + (-36x^3 - 30x^2 - 18x - 2)          (k = 1)
//   BLS12-381 3 (q^4 - q^2 + 1) / r = (x - 1)^2 (x + q) (x^2 + q^2 - 1) + 3                                                   (k = 3)
// tools/gen_pairing_constants.py asserts both identities in integers and emits k as C::GT_POWER.  Fq's inversion maps 0 to 0, so
// final_exp(0) = 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ZKP_PAIR_INL __host__ __device__ __forceinline__
#define ZKP_PAIR_FN __host__ __device__ __attribute__((noinline))
#else
#define ZKP_PAIR_INL inline
#define ZKP_PAIR_FN
#endif

namespace zkp {

template <class C, class F2>
struct Pairing {
  using B = typename F2::B;
  struct F6 {
    F2 c0, c1, c2;
  };
  struct F12 {
    F6 c0, c1;
  };
  static constexpr int FQ_WORDS = C::Fq::N;
  static constexpr int F12_WORDS = 12 * FQ_WORDS;

  // ------------------------------------------------------------------------------------------- constants
  static ZKP_PAIR_INL B fq_const(const uint32_t* w) {
    B r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < FQ_WORDS; i++) r.v[i] = w[i];
    return r;
  }
  static ZKP_PAIR_INL F2 fq2_const(const uint32_t (*w)[FQ_WORDS]) { return F2{fq_const(w[0]), fq_const(w[1])}; }

  // ------------------------------------------------------------------------------------------- Fq2 helpers
  static ZKP_PAIR_INL F2 mul_xi(const F2& a) {               // a (XI0 + u)
    if constexpr (C::XI0 == 1) {
      return F2{a.c0 - a.c1, a.c0 + a.c1};
    } else {
      static_assert(C::XI0 == 1 || C::XI0 == 9, "xi = 1 + u or 9 + u");
      const F2 a9 = a.dbl().dbl().dbl() + a;
      return F2{a9.c0 - a.c1, a9.c1 + a.c0};
    }
  }
  static ZKP_PAIR_INL F2 scale(const F2& a, const B& k) { return F2{a.c0 * k, a.c1 * k}; }
  static ZKP_PAIR_INL F2 conj2(const F2& a) { return F2{a.c0, a.c1.neg()}; }
  static ZKP_PAIR_INL F2 triple(const F2& a) { return a.dbl() + a; }

  // ------------------------------------------------------------------------------------------- Fq6
  static ZKP_PAIR_INL F6 zero6() { return F6{F2::zero(), F2::zero(), F2::zero()}; }
  static ZKP_PAIR_INL F6 one6() { return F6{F2::one(), F2::zero(), F2::zero()}; }
  static ZKP_PAIR_INL F6 add6(const F6& a, const F6& b) { return F6{a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2}; }
  static ZKP_PAIR_INL F6 sub6(const F6& a, const F6& b) { return F6{a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2}; }
  static ZKP_PAIR_INL F6 neg6(const F6& a) { return F6{a.c0.neg(), a.c1.neg(), a.c2.neg()}; }
  static ZKP_PAIR_INL F6 mulv6(const F6& a) { return F6{mul_xi(a.c2), a.c0, a.c1}; }
  // Karatsuba: 6 Fq2 products
  static ZKP_PAIR_FN void mul6(F6& r, const F6& a, const F6& b) {
    const F2 v0 = a.c0 * b.c0, v1 = a.c1 * b.c1, v2 = a.c2 * b.c2;
    const F2 t0 = (a.c1 + a.c2) * (b.c1 + b.c2) - v1 - v2;
    const F2 t1 = (a.c0 + a.c1) * (b.c0 + b.c1) - v0 - v1;
    const F2 t2 = (a.c0 + a.c2) * (b.c0 + b.c2) - v0 - v2;
    r.c0 = v0 + mul_xi(t0);
    r.c1 = t1 + mul_xi(v2);
    r.c2 = t2 + v1;
  }
  // a (c0 + c1 v): 5 Fq2 products
  static ZKP_PAIR_FN void mul6_by_01(F6& r, const F6& s, const F2& c0, const F2& c1) {
    const F2 aa = s.c0 * c0, bb = s.c1 * c1;
    const F2 t1 = mul_xi((s.c1 + s.c2) * c1 - bb) + aa;
    const F2 t3 = (s.c0 + s.c2) * c0 - aa + bb;
    const F2 t2 = (c0 + c1) * (s.c0 + s.c1) - aa - bb;
    r.c0 = t1;
    r.c1 = t2;
    r.c2 = t3;
  }
  static ZKP_PAIR_FN void inv6(F6& r, const F6& a) {
    const F2 t0 = a.c0.sqr() - mul_xi(a.c1 * a.c2);
    const F2 t1 = mul_xi(a.c2.sqr()) - a.c0 * a.c1;
    const F2 t2 = a.c1.sqr() - a.c0 * a.c2;
    const F2 d = (a.c0 * t0 + mul_xi(a.c2 * t1 + a.c1 * t2)).inv();
    r.c0 = t0 * d;
    r.c1 = t1 * d;
    r.c2 = t2 * d;
  }

  // ------------------------------------------------------------------------------------------- Fq12
  static ZKP_PAIR_INL F12 one12() { return F12{one6(), zero6()}; }
  static ZKP_PAIR_INL F12 conj12(const F12& a) { return F12{a.c0, neg6(a.c1)}; }
  // r may be a or b
  static ZKP_PAIR_FN void mul12(F12& r, const F12& a, const F12& b) {
    F6 v0, v1, s;
    mul6(v0, a.c0, b.c0);
    mul6(v1, a.c1, b.c1);
    mul6(s, add6(a.c0, a.c1), add6(b.c0, b.c1));
    r.c1 = sub6(sub6(s, v0), v1);
    r.c0 = add6(v0, mulv6(v1));
  }
  static ZKP_PAIR_FN void sqr12(F12& r, const F12& a) {
    F6 ab, s;
    mul6(ab, a.c0, a.c1);
    mul6(s, add6(a.c0, a.c1), add6(a.c0, mulv6(a.c1)));
    r.c0 = sub6(sub6(s, ab), mulv6(ab));
    r.c1 = add6(ab, ab);
  }
  static ZKP_PAIR_FN void inv12(F12& r, const F12& a) {
    F6 t, u;
    mul6(t, a.c0, a.c0);
    mul6(u, a.c1, a.c1);
    t = sub6(t, mulv6(u));
    inv6(u, t);
    mul6(t, a.c1, u);
    mul6(r.c0, a.c0, u);
    r.c1 = neg6(t);
  }
  // a^(q^k), k = 1, 2, 3
  static ZKP_PAIR_FN void frob12(F12& r, const F12& a, int k) {
    auto one = [&](const F2& x, int j, int i) {
      const F2 y = (k & 1) ? conj2(x) : x;
      return y * fq2_const(C::FROB[k - 1][2 * i + j]);
    };
    r.c0.c0 = one(a.c0.c0, 0, 0);
    r.c0.c1 = one(a.c0.c1, 0, 1);
    r.c0.c2 = one(a.c0.c2, 0, 2);
    r.c1.c0 = one(a.c1.c0, 1, 0);
    r.c1.c1 = one(a.c1.c1, 1, 1);
    r.c1.c2 = one(a.c1.c2, 1, 2);
  }
  // f (A + B w), A = a0 + a1 v, B = b0 + b1 v: three products by (c0, c1, 0), 15 Fq2 products
  static ZKP_PAIR_FN void mul12_by_line(F12& f, const F2& a0, const F2& a1, const F2& b0, const F2& b1) {
    F6 v0, v1, s;
    mul6_by_01(v0, f.c0, a0, a1);
    mul6_by_01(v1, f.c1, b0, b1);
    mul6_by_01(s, add6(f.c0, f.c1), a0 + b0, a1 + b1);
    f.c1 = sub6(sub6(s, v0), v1);
    f.c0 = add6(v0, mulv6(v1));
  }
  // (x + y s)^2 in Fq4 = Fq2[s] / (s^2 - xi)
  static ZKP_PAIR_INL void sqr4(F2& t0, F2& t1, const F2& x, const F2& y) {
    const F2 t = x * y;
    t0 = (x + y) * (mul_xi(y) + x) - t - mul_xi(t);
    t1 = t.dbl();
  }
  // Granger-Scott: a^2 for a in the cyclotomic subgroup (a^(q^6 + 1) = ... = 1 after the easy part), 6 Fq2 products + 3 squarings' worth
  static ZKP_PAIR_FN void cyc_sqr12(F12& r, const F12& a) {
    F2 t0, t1, t2, t3, t4, t5;
    sqr4(t0, t1, a.c0.c0, a.c1.c1);
    sqr4(t2, t3, a.c1.c0, a.c0.c2);
    sqr4(t4, t5, a.c0.c1, a.c1.c2);
    const F2 x5 = mul_xi(t5);
    const F2 z0 = a.c0.c0, z4 = a.c0.c1, z3 = a.c0.c2, z2 = a.c1.c0, z1 = a.c1.c1, z5 = a.c1.c2;
    r.c0.c0 = (t0 - z0).dbl() + t0;
    r.c1.c1 = (t1 + z1).dbl() + t1;
    r.c1.c0 = (x5 + z2).dbl() + x5;
    r.c0.c2 = (t4 - z3).dbl() + t4;
    r.c0.c1 = (t2 - z4).dbl() + t2;
    r.c1.c2 = (t3 + z5).dbl() + t3;
  }
  static constexpr int top_bit(uint64_t v) {
    int b = 0;
    while (v >> 1) {
      v >>= 1;
      b++;
    }
    return b;
  }
  // a^x for a in the cyclotomic subgroup (the inverse is the conjugate there)
  static ZKP_PAIR_FN void pow_x(F12& r, const F12& a) {
    F12 t = a;
    for (int i = top_bit(C::ABS_X) - 1; i >= 0; i--) {
      cyc_sqr12(t, t);
      if ((C::ABS_X >> i) & 1) mul12(t, t, a);
    }
    r = C::X_NEG ? conj12(t) : t;
  }
  static ZKP_PAIR_INL bool is_one12(const F12& a) {
    return a.c0.c0 == F2::one() && a.c0.c1.is_zero() && a.c0.c2.is_zero() && a.c1.c0.is_zero() && a.c1.c1.is_zero() && a.c1.c2.is_zero();
  }

  // ------------------------------------------------------------------------------------------- final exponentiation
  // f^(GT_POWER (q^12 - 1) / r); in place
  static ZKP_PAIR_FN void final_exp(F12& f) {
    F12 t, u;
    inv12(t, f);
    mul12(f, conj12(f), t);              // f^(q^6 - 1)
    frob12(t, f, 2);
    mul12(f, t, f);                      // ^(q^2 + 1): f is in the cyclotomic subgroup from here on
    if constexpr (C::BN) {
      F12 a, b, c, y;
      pow_x(a, f);
      pow_x(b, a);
      pow_x(c, b);
      // y = c^36
      cyc_sqr12(y, c);
      cyc_sqr12(y, y);
      cyc_sqr12(y, y);
      mul12(y, y, c);
      cyc_sqr12(y, y);
      cyc_sqr12(y, y);
      // t = b^6, u = b^12
      cyc_sqr12(t, b);
      mul12(t, t, b);
      cyc_sqr12(t, t);
      cyc_sqr12(u, t);
      // c <- f^(q^3) (f b^6)^(q^2): c is free
      mul12(c, t, f);
      frob12(c, c, 2);
      frob12(b, f, 3);
      mul12(c, c, b);
      // b <- b^18, y <- c^36 b^18, u <- c^36 b^30
      mul12(b, u, t);
      mul12(y, y, b);
      mul12(u, y, u);
      // t = a^6, b = a^12
      cyc_sqr12(t, a);
      mul12(t, t, a);
      cyc_sqr12(t, t);
      cyc_sqr12(b, t);
      // y <- (conj(c^36 b^18 a^12) f)^q
      mul12(y, y, b);
      mul12(y, conj12(y), f);
      frob12(y, y, 1);
      // u <- conj(c^36 b^30 a^18 f^2)
      mul12(b, b, t);
      mul12(u, u, b);
      cyc_sqr12(t, f);
      mul12(u, u, t);
      mul12(f, c, y);
      mul12(f, f, conj12(u));
    } else {
      F12 y;
      pow_x(y, f);
      mul12(y, y, conj12(f));            // f^(x - 1)
      pow_x(t, y);
      mul12(y, t, conj12(y));            // f^((x - 1)^2)
      pow_x(t, y);
      frob12(u, y, 1);
      mul12(y, t, u);                    // ^(x + q)
      pow_x(t, y);
      pow_x(t, t);
      frob12(u, y, 2);
      mul12(t, t, u);
      mul12(t, t, conj12(y));            // ^(x^2 + q^2 - 1)
      cyc_sqr12(u, f);
      mul12(u, u, f);
      mul12(f, t, u);                    // f^3
    }
  }

  // ------------------------------------------------------------------------------------------- Miller loop
  struct Twist {
    F2 x, y, z;
  };
  struct Line {
    F2 c0, c1, c2;
  };
  static ZKP_PAIR_FN void dbl_step(Twist& r, Line& l) {
    const B two_inv = fq_const(C::TWO_INV);
    const F2 a = scale(r.x * r.y, two_inv);
    const F2 b = r.y.sqr(), c = r.z.sqr();
    const F2 e = fq2_const(C::TWIST_B) * triple(c);
    const F2 f = triple(e);
    const F2 g = scale(b + f, two_inv);
    const F2 h = (r.y + r.z).sqr() - (b + c);
    const F2 i = e - b;
    const F2 j = r.x.sqr();
    const F2 e2 = e.sqr();
    r.x = a * (b - f);
    r.y = g.sqr() - triple(e2);
    r.z = b * h;
    if constexpr (C::TWIST_D) {
      l = Line{h.neg(), triple(j), i};
    } else {
      l = Line{i, triple(j), h.neg()};
    }
  }
  static ZKP_PAIR_FN void add_step(Twist& r, Line& l, const F2& qx, const F2& qy) {
    const F2 theta = r.y - qy * r.z;
    const F2 lambda = r.x - qx * r.z;
    const F2 c = theta.sqr(), d = lambda.sqr();
    const F2 e = lambda * d;
    const F2 f = r.z * c;
    const F2 g = r.x * d;
    const F2 h = e + f - g.dbl();
    r.x = lambda * h;
    r.y = theta * (g - h) - e * r.y;
    r.z = r.z * e;
    const F2 j = theta * qx - lambda * qy;
    if constexpr (C::TWIST_D) {
      l = Line{lambda, theta.neg(), j};
    } else {
      l = Line{j, theta.neg(), lambda};
    }
  }
  // f <- f line(P)
  static ZKP_PAIR_INL void ell(F12& f, const Line& l, const B& px, const B& py) {
    if constexpr (C::TWIST_D) {
      mul12_by_line(f, scale(l.c0, py), F2::zero(), scale(l.c1, px), l.c2);
    } else {
      mul12_by_line(f, l.c0, scale(l.c1, px), F2::zero(), scale(l.c2, py));
    }
  }
  // the Miller function of the optimal-ate pairing at (P, Q), P = (px, py) in G1 and Q = (qx, qy) in G2, neither the identity
  static ZKP_PAIR_FN void miller(F12& f, const B& px, const B& py, const F2& qx, const F2& qy) {
    f = one12();
    Twist t{qx, qy, F2::one()};
    Line l;
    for (int i = C::LOOP_BITS - 2; i >= 0; i--) {
      sqr12(f, f);
      dbl_step(t, l);
      ell(f, l, px, py);
      if ((C::LOOP[i >> 5] >> (i & 31)) & 1) {
        add_step(t, l, qx, qy);
        ell(f, l, px, py);
      }
    }
    if constexpr (C::BN) {
      const F2 gx = fq2_const(C::TWIST_FROB_X), gy = fq2_const(C::TWIST_FROB_Y);
      const F2 q1x = conj2(qx) * gx, q1y = conj2(qy) * gy;
      const F2 q2x = conj2(q1x) * gx, q2y = (conj2(q1y) * gy).neg();
      add_step(t, l, q1x, q1y);
      ell(f, l, px, py);
      add_step(t, l, q2x, q2y);
      ell(f, l, px, py);
    } else {
      f = conj12(f);
    }
  }
};

}  // namespace zkp
