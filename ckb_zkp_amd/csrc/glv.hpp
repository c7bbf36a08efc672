// GLV decomposition of a G1 scalar (both curves have j = 0: phi(x, y) = (beta x, y) is an endomorphism with phi(P) = lambda P).
// Shared by the Groth16 assembly kernel (msm_group.hip) and the IPA generator fold (ipa.hip, which decomposes its two uniform
// scalars once per call on the host).  k = k1 + k2 lambda (mod r) with |k1|, |k2| < 2^129 (glv_constants.inc, generated and
// checked by tools/gen_glv.py).
#pragma once
#include "field_dev.hpp"

namespace zkp {

#define ZKP_HD_INLINE __host__ __device__ __forceinline__

#include "glv_constants.inc"
// c = (k * g) >> 256, k: 8 words, g: 5 words
ZKP_HD_INLINE void glv_mulhi(const uint32_t* k, const uint32_t* g, uint32_t* c) {
  uint32_t t[13];
#pragma unroll
  for (int i = 0; i < 13; i++) t[i] = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint64_t x = (uint64_t)k[i] * g[j] + t[i + j] + carry;
      t[i + j] = (uint32_t)x;
      carry = x >> 32;
    }
    t[8 + j] = (uint32_t)carry;
  }
#pragma unroll
  for (int i = 0; i < 5; i++) c[i] = t[8 + i];
}
// acc (10 words, two's complement) += sign * x * y  (x, y: 5-word magnitudes; neg != 0 subtracts)
ZKP_HD_INLINE void glv_mac(uint32_t* acc, const uint32_t* x, const uint32_t* y, int neg) {
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
      uint64_t v = (uint64_t)x[i] * y[j] + t[i + j] + carry;
      t[i + j] = (uint32_t)v;
      carry = v >> 32;
    }
    t[5 + j] = (uint32_t)carry;
  }
  uint64_t c = neg ? 1 : 0;                                 // subtract = add the two's complement
#pragma unroll
  for (int i = 0; i < 10; i++) {
    c += (uint64_t)acc[i] + (neg ? ~t[i] : t[i]);
    acc[i] = (uint32_t)c;
    c >>= 32;
  }
}
// 10-word two's complement -> 5-word magnitude + sign
ZKP_HD_INLINE int glv_abs(uint32_t* acc, uint32_t* out) {
  const int neg = (int)(acc[9] >> 31);
  uint64_t c = neg ? 1 : 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    c += neg ? (uint32_t)~acc[i] : acc[i];
    acc[i] = (uint32_t)c;
    c >>= 32;
  }
#pragma unroll
  for (int i = 0; i < 5; i++) out[i] = acc[i];
  return neg;
}
// k (canonical scalar, 8 words) -> |k1|, |k2| < 2^BITS and their signs: k = k1 + k2 lambda (mod r).  The identity holds for ANY
// integers c1, c2 (a_i + b_i lambda = 0 mod r), so the truncated quotients only cost a bit of size (gen_glv.py checks the bound).
template <class G>
ZKP_HD_INLINE void glv_decompose(const uint32_t* k, uint32_t* k1, int* neg1, uint32_t* k2, int* neg2) {
  uint32_t g1[5], g2[5], a1[5], b1[5], a2[5], b2[5], c1[5], c2[5];
#pragma unroll
  for (int i = 0; i < 5; i++) {
    g1[i] = G::G1[i]; g2[i] = G::G2[i]; a1[i] = G::A1[i]; b1[i] = G::B1[i]; a2[i] = G::A2[i]; b2[i] = G::B2[i];
  }
  glv_mulhi(k, g1, c1);                                     // |c1|, sign G1_NEG
  glv_mulhi(k, g2, c2);
  uint32_t acc[10];
#pragma unroll
  for (int i = 0; i < 10; i++) acc[i] = i < 8 ? k[i] : 0;
  glv_mac(acc, c1, a1, !(G::G1_NEG ^ G::A1_NEG));           // k1 = k - c1 a1 - c2 a2
  glv_mac(acc, c2, a2, !(G::G2_NEG ^ G::A2_NEG));
  *neg1 = glv_abs(acc, k1);
#pragma unroll
  for (int i = 0; i < 10; i++) acc[i] = 0;
  glv_mac(acc, c1, b1, !(G::G1_NEG ^ G::B1_NEG));           // k2 = -c1 b1 - c2 b2
  glv_mac(acc, c2, b2, !(G::G2_NEG ^ G::B2_NEG));
  *neg2 = glv_abs(acc, k2);
}


}  // namespace zkp
