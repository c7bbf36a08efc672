// IPA generator fold (ipa.hip): digit plan and the per-curve launch table.  Kept apart from MsmVtbl / MsmSmallVtbl so that the
// MSM units are not touched by it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

constexpr int IPA_LANES = 64;             // one wave per workgroup: one batch inversion per 64 outputs
constexpr int IPA_MAX_DIG = 136;          // joint digit positions: GLV magnitudes < 2^129 -> joint sparse form of <= 130 digits

// the joint digits of a = k1 + k2 lambda and b = k3 + k4 lambda, most significant last; one byte per position: low nibble the
// (L, phi L) digit, high nibble the (R, phi R) digit, coded as in ipa.hip.  A kernel argument: the same for every lane.
struct IpaPlan {
  uint32_t ndig;
  uint8_t dig[IPA_MAX_DIG];
};

struct IpaVtbl {
  // zkp_g1_ipa_fold_dev after its NULL checks: checks the rest, plans on the host, one launch, returns when out is written
  void (*fold)(zkp_ctx* ctx, const uint64_t* l_xy, const uint8_t* l_inf, const uint64_t* r_xy, const uint8_t* r_inf, size_t n,
               const uint64_t* a_host, const uint64_t* b_host, uint64_t* out_xy, uint8_t* out_inf);
};

const IpaVtbl* ipa_vtbl_c0();             // ipa.hip, -DZKP_CFG_CURVE=0
const IpaVtbl* ipa_vtbl_c1();             // ipa.hip, -DZKP_CFG_CURVE=1
inline const IpaVtbl* ipa_vtbl(int curve) {
  if (curve == ZKP_BN254) return ipa_vtbl_c0();
  if (curve == ZKP_BLS12_381) return ipa_vtbl_c1();
  throw StatusError{ZKP_ERR_UNSUPPORTED_CURVE};
}

}  // namespace zkp
