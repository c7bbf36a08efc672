// Optimal-ate pairings on the device (pairing.hip, compiled once per curve): products of Miller functions per group of pairs, the
// final exponentiation, and the per-curve launch table.  Kept apart from the other launch tables so that no other unit is touched.
//
// Contract of the final exponentiation: out = f^(k (q^12 - 1) / r) with k = PAIRING_GT_POWER_* below, fixed at compile time and
// coprime to r: 1 on BN254 (an exact chain), 3 on BLS12-381 (the usual chain); zkp_pairing_info returns it.  So a pairing value is
// e(P, Q)^k: equality tests and product-equals-one tests are unaffected; compare GT values only with GT values of this library.
// An input of 0 gives 0 (Fq's inversion maps 0 to 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

constexpr int PAIRING_LANES = 64;                        // pairs of one workgroup: one wave, one pair (or one Fq12) per lane
constexpr size_t PAIRING_MAX_N = (size_t)1 << 20;        // == ZKP_PAIRING_MAX_N
constexpr uint64_t PAIRING_GT_POWER_BN254 = 1;
constexpr uint64_t PAIRING_GT_POWER_BLS12_381 = 3;
static_assert(PAIRING_MAX_N == ZKP_PAIRING_MAX_N, "pairing.hpp and zkp_accel.h disagree");

struct PairingVtbl {
  // zkp_pairing_info: k, u64 words per Fq12, pairs per workgroup, largest n, LDS bytes of the Miller kernel; no device
  void (*info)(uint64_t* info);
  // the device entries after their NULL checks: check the rest, then only launch on the context's current stream
  void (*miller)(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n,
                 size_t group, uint64_t* out_f12);
  void (*final_exp)(zkp_ctx* ctx, const uint64_t* f12, size_t m, uint64_t* out_gt);
  void (*product_is_one)(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                         size_t n, size_t group, uint8_t* ok);
  // the host-pointer conveniences: stage, run, copy back, synchronise.  gt_out: n Fq12 (one pairing each); ok_out: n / group bytes
  void (*pairing_host)(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                       size_t n, uint64_t* gt_out);
  void (*check_host)(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                     size_t n, size_t group, uint8_t* ok_out);
};

const PairingVtbl* pairing_vtbl_c0();     // pairing.hip, -DZKP_CFG_CURVE=0
const PairingVtbl* pairing_vtbl_c1();     // pairing.hip, -DZKP_CFG_CURVE=1
inline const PairingVtbl* pairing_vtbl(int curve) {
  if (curve == ZKP_BN254) return pairing_vtbl_c0();
  if (curve == ZKP_BLS12_381) return pairing_vtbl_c1();
  throw StatusError{ZKP_ERR_BAD_ARG};
}

}  // namespace zkp
