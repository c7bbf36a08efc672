// PLONK prover rounds 2 and 3 on the device (plonk.hip): the running product over Fr, the permutation accumulator z of
// PermutationKey::compute_z and the fused third-round quotient.  The host entries behind zkp_fr_prefix_product_dev /
// zkp_fr_plonk_perm_z_dev / zkp_fr_plonk_quotient_dev.  Fr only: one object serves both curves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

// The running product is blocked: one workgroup of PLONK_SCAN_THREADS threads owns PLONK_SCAN_BLOCK consecutive elements,
// PLONK_SCAN_ITEMS per thread.  More than one block: the blocks' totals are scanned the same way (a level), recursively.
constexpr uint32_t PLONK_SCAN_THREADS = 256;
constexpr uint32_t PLONK_SCAN_ITEMS = 4;
constexpr uint32_t PLONK_SCAN_BLOCK = 1024;
static_assert(PLONK_SCAN_BLOCK == PLONK_SCAN_THREADS * PLONK_SCAN_ITEMS, "a block is its threads' items");
constexpr uint32_t PLONK_SCAN_MAX_LOG = 30;        // n <= 2^30: three levels at most
// The quotient kernel's grid is capped: thread j owns the points j, j + T, j + 2T, ... with T = min(4n, THREADS * MAX_BLOCKS).
constexpr uint32_t PLONK_QUOT_THREADS = 256;
constexpr uint32_t PLONK_QUOT_MAX_BLOCKS = 512;

// after the NULL checks of capi.hip: every other rule, then the work; each returns when its outputs are written
void fr_prefix_product(zkp_ctx* ctx, int curve, const uint64_t* in_dev, uint64_t* out_dev, size_t n, uint64_t* total_out_host);
void fr_plonk_perm_z(zkp_ctx* ctx, int curve, const uint64_t* const* w_dev, const uint64_t* const* sigma_dev, uint32_t log_n,
                     const uint64_t* ks_host, const uint64_t* beta_host, const uint64_t* gamma_host, uint64_t* z_out_dev,
                     int32_t* closes_out_host);
void fr_plonk_quotient(zkp_ctx* ctx, int curve, const uint64_t* const* w_4n, const uint64_t* z_4n, const uint64_t* pi_4n,
                       const uint64_t* const* q_4n, const uint64_t* const* sigma_4n, const uint64_t* l1_4n, uint32_t log_n,
                       const uint64_t* ks_host, const uint64_t* beta_host, const uint64_t* gamma_host, const uint64_t* alpha_host,
                       uint64_t* t_out_dev);

}  // namespace zkp
