// Transforms over G1 points (g1_ntt.hip): per-lane scalar multiplication, the radix-2 butterfly network over curve points and the
// per-curve launch table.  Kept apart from MsmVtbl / MsmSmallVtbl / IpaVtbl so that those units are not touched by it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

constexpr int G1N_LANES = 64;             // one wave per workgroup: one batch inversion per 64 lanes (64 / 128 output points)
constexpr int G1N_MAX_LOG = 24;           // == ZKP_G1_NTT_MAX_LOG; <= the two-adicity of both scalar fields (28 / 32)
constexpr int G1N_SCALAR_BITS = 256;      // canonical scalar words walked by the window recoding
constexpr int G1N_LDS_BYTES = 160 * 1024; // LDS of one CU: bounds lanes x window table
static_assert(G1N_MAX_LOG == ZKP_G1_NTT_MAX_LOG, "g1_ntt.hpp and zkp_accel.h disagree");

struct G1NttVtbl {
  // zkp_g1_scale_vec_dev after its NULL checks: checks the rest, one launch
  void (*scale_vec)(zkp_ctx* ctx, const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t* out_xy,
                    uint8_t* out_inf);
  // zkp_g1_ntt_dev after its NULL checks: checks the rest, log_n + 2 launches (+ 1 for the inverse's 1 / n)
  void (*ntt)(zkp_ctx* ctx, uint64_t* xy, uint8_t* inf, uint32_t log_n, int32_t op);
};

const G1NttVtbl* g1_ntt_vtbl_c0();        // g1_ntt.hip, -DZKP_CFG_CURVE=0
const G1NttVtbl* g1_ntt_vtbl_c1();        // g1_ntt.hip, -DZKP_CFG_CURVE=1
inline const G1NttVtbl* g1_ntt_vtbl(int curve) {
  if (curve == ZKP_BN254) return g1_ntt_vtbl_c0();
  if (curve == ZKP_BLS12_381) return g1_ntt_vtbl_c1();
  throw StatusError{ZKP_ERR_BAD_ARG};
}

}  // namespace zkp
