// aSVC subvector commitments (asvc/src/lib.rs): the Fr work of prove_pos between its inverse transform and its MSM, the quotient
// of Phi(X) by the subvector's vanishing polynomial A_I(X) = prod_{i in I} (X - w^i), and the weights 1 / A_I'(w^i) that
// aggregate_proofs uses (asvc.hip).  The host entries behind zkp_fr_asvc_subset_weights_dev / zkp_fr_asvc_quotient_dev.
// Fr only: one object serves both curves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

// Positions of one call: the per-position constants stay small enough to sit in cache for every pass (== ZKP_ASVC_MAX_POSITIONS).
constexpr uint32_t ASVC_MAX_POSITIONS = 1024;
// Workgroup of every kernel of the unit.
constexpr uint32_t ASVC_THREADS = 256;
// Positions whose running values one thread of the segment-head pass keeps in registers: a coefficient is loaded once per group.
constexpr uint32_t ASVC_GROUP = 4;
// Consecutive quotient coefficients one thread of the output pass accumulates in registers over all positions.
constexpr uint32_t ASVC_SPAN = 8;
// The scan over segment heads is blocked like poly.hip's Horner scan: ASVC_CHUNK heads per thread, ASVC_THREADS chunks per tile.
constexpr uint32_t ASVC_CHUNK = 32;
constexpr uint32_t ASVC_TILE = ASVC_CHUNK * ASVC_THREADS;
// Domains: 2^1 .. 2^min(ASVC_MAX_LOG, two-adicity), the limits of zkp_ntt_dev.
constexpr uint32_t ASVC_MAX_LOG = 30;
static_assert(ASVC_MAX_POSITIONS == ZKP_ASVC_MAX_POSITIONS, "the header quotes the same cap");
static_assert(ASVC_TILE == 8192 && (ASVC_SPAN & (ASVC_SPAN - 1)) == 0, "asvc.hip shifts by these");

// after the NULL checks of capi.hip: every other rule, then the work
void asvc_subset_weights(zkp_ctx* ctx, int curve, uint32_t log_n, const uint32_t* positions_host, size_t k, uint64_t* weights_dev,
                         uint64_t* weights_host);                 // with weights_host: returns when it is written
void asvc_quotient(zkp_ctx* ctx, int curve, const uint64_t* phi_dev, uint32_t log_n, const uint32_t* positions_host, size_t k,
                   uint64_t* q_dev);                              // launches only, like fr_vec_op

}  // namespace zkp
