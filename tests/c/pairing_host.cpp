// CPU run of ckb_zkp_amd/csrc/pairing_dev.hpp: the tower, the Miller loop and the final exponentiation instantiated with a plain C++
// Montgomery field in place of the device's Fp2<P>.  tests/test_pairing_ref.py feeds it points and Fq12 elements as Montgomery words
// and compares what comes back with Python integers, so a wrong formula or constant shows without a device.
//
//   pairing_host <curve 0|1>      stdin, one request per line, words as 8-digit hex, least significant first:
//     P <2 N words G1> <4 N words G2>     -> final_exp(miller(P, Q)), 12 N words
//     M <2 N words G1> <4 N words G2>     -> miller(P, Q)
//     F <12 N words>                      -> final_exp(f)
//     X <12 N words> <12 N words>         -> the product
//     C <2 N words G1> <4 N words G2>     -> two decimal numbers: the Fq products of miller(P, Q) and of the final exponentiation
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace zkp {
#include "field_constants.inc"
#include "pairing_constants.inc"
}  // namespace zkp
#include "pairing_dev.hpp"

static unsigned long long g_products = 0;      // Fq products (squarings included) since the program started

template <class P>
struct HFp {
  static constexpr int N = P::N;
  uint32_t v[N];
  static HFp zero() {
    HFp r;
    for (int i = 0; i < N; i++) r.v[i] = 0;
    return r;
  }
  static HFp one() {
    HFp r;
    for (int i = 0; i < N; i++) r.v[i] = P::ONE[i];
    return r;
  }
  bool is_zero() const {
    uint32_t o = 0;
    for (int i = 0; i < N; i++) o |= v[i];
    return o == 0;
  }
  bool operator==(const HFp& b) const { return memcmp(v, b.v, sizeof v) == 0; }
  static bool geq(const uint32_t* a) {
    for (int i = N - 1; i >= 0; i--)
      if (a[i] != P::MOD[i]) return a[i] > P::MOD[i];
    return true;
  }
  static void sub_mod(uint32_t* a) {
    uint64_t br = 0;
    for (int i = 0; i < N; i++) {
      const uint64_t d = (uint64_t)a[i] - P::MOD[i] - br;
      a[i] = (uint32_t)d;
      br = (d >> 63) & 1;
    }
  }
  friend HFp operator+(const HFp& a, const HFp& b) {
    HFp r;
    uint64_t c = 0;
    for (int i = 0; i < N; i++) {
      c += (uint64_t)a.v[i] + b.v[i];
      r.v[i] = (uint32_t)c;
      c >>= 32;
    }
    if (c || geq(r.v)) sub_mod(r.v);
    return r;
  }
  HFp neg() const {
    if (is_zero()) return *this;
    HFp r;
    uint64_t br = 0;
    for (int i = 0; i < N; i++) {
      const uint64_t d = (uint64_t)P::MOD[i] - v[i] - br;
      r.v[i] = (uint32_t)d;
      br = (d >> 63) & 1;
    }
    return r;
  }
  friend HFp operator-(const HFp& a, const HFp& b) { return a + b.neg(); }
  HFp dbl() const { return *this + *this; }
  friend HFp operator*(const HFp& a, const HFp& b) {           // CIOS
    g_products++;
    uint32_t t[N + 2] = {0};
    for (int i = 0; i < N; i++) {
      uint64_t c = 0;
      for (int j = 0; j < N; j++) {
        c += (uint64_t)a.v[j] * b.v[i] + t[j];
        t[j] = (uint32_t)c;
        c >>= 32;
      }
      c += t[N];
      t[N] = (uint32_t)c;
      t[N + 1] = (uint32_t)(c >> 32);
      const uint32_t m = t[0] * P::INV;
      c = ((uint64_t)m * P::MOD[0] + t[0]) >> 32;
      for (int j = 1; j < N; j++) {
        c += (uint64_t)m * P::MOD[j] + t[j];
        t[j - 1] = (uint32_t)c;
        c >>= 32;
      }
      c += t[N];
      t[N - 1] = (uint32_t)c;
      t[N] = t[N + 1] + (uint32_t)(c >> 32);
    }
    if (t[N] || geq(t)) sub_mod(t);
    HFp r;
    memcpy(r.v, t, sizeof r.v);
    return r;
  }
  HFp sqr() const { return *this * *this; }
  HFp inv() const {                                             // Fermat, 0 -> 0 as on the device
    HFp r = one();
    for (int bit = 32 * N - 1; bit >= 0; bit--) {
      r = r.sqr();
      if ((P::PM2[bit >> 5] >> (bit & 31)) & 1) r = r * *this;
    }
    return r;
  }
};

template <class P>
struct HFp2 {
  using B = HFp<P>;
  B c0, c1;
  static HFp2 zero() { return {B::zero(), B::zero()}; }
  static HFp2 one() { return {B::one(), B::zero()}; }
  bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
  bool operator==(const HFp2& o) const { return c0 == o.c0 && c1 == o.c1; }
  friend HFp2 operator+(const HFp2& a, const HFp2& b) { return {a.c0 + b.c0, a.c1 + b.c1}; }
  friend HFp2 operator-(const HFp2& a, const HFp2& b) { return {a.c0 - b.c0, a.c1 - b.c1}; }
  HFp2 neg() const { return {c0.neg(), c1.neg()}; }
  HFp2 dbl() const { return {c0.dbl(), c1.dbl()}; }
  // the device's formulas (field_dev.hpp Fp2), so that the product counts are the device's: Karatsuba, complex squaring
  friend HFp2 operator*(const HFp2& a, const HFp2& b) {
    const B v0 = a.c0 * b.c0, v1 = a.c1 * b.c1;
    const B s = (a.c0 + a.c1) * (b.c0 + b.c1);
    return {v0 - v1, s - v0 - v1};
  }
  HFp2 sqr() const {
    const B t = c0 * c1;
    return {(c0 + c1) * (c0 - c1), t.dbl()};
  }
  HFp2 inv() const {
    const B n = (c0.sqr() + c1.sqr()).inv();
    return {c0 * n, (c1 * n).neg()};
  }
};

template <class C>
int run() {
  using F2 = HFp2<typename C::Fq>;
  using PR = zkp::Pairing<C, F2>;
  using F12 = typename PR::F12;
  constexpr int N = C::Fq::N;
  static_assert(sizeof(F12) == 12 * N * 4, "an Fq12 is 12 N words without padding");
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, tok;
    in >> op;
    std::vector<uint32_t> w;
    while (in >> tok) w.push_back((uint32_t)strtoul(tok.c_str(), nullptr, 16));
    F12 f;
    if (op == "P" || op == "M" || op == "C") {
      if (w.size() != (size_t)6 * N) return 2;
      typename F2::B px, py;
      F2 qx, qy;
      memcpy(px.v, &w[0], 4 * N);
      memcpy(py.v, &w[N], 4 * N);
      memcpy(&qx, &w[2 * N], 8 * N);
      memcpy(&qy, &w[4 * N], 8 * N);
      const unsigned long long c0 = g_products;
      PR::miller(f, px, py, qx, qy);
      const unsigned long long c1 = g_products;
      if (op != "M") PR::final_exp(f);
      if (op == "C") {
        printf("%llu %llu\n", c1 - c0, g_products - c1);
        continue;
      }
    } else if (op == "F") {
      if (w.size() != (size_t)12 * N) return 2;
      memcpy(&f, w.data(), sizeof f);
      PR::final_exp(f);
    } else if (op == "X") {
      if (w.size() != (size_t)24 * N) return 2;
      F12 a, b;
      memcpy(&a, w.data(), sizeof a);
      memcpy(&b, w.data() + 12 * N, sizeof b);
      PR::mul12(f, a, b);
    } else {
      return 2;
    }
    uint32_t out[12 * N];
    memcpy(out, &f, sizeof f);
    for (int i = 0; i < 12 * N; i++) printf("%08x%c", out[i], i + 1 == 12 * N ? '\n' : ' ');
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  return argv[1][0] == '0' ? run<zkp::Bn254Pairing>() : run<zkp::Bls381Pairing>();
}
