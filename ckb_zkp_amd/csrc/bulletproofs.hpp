// The Fr work of the Bulletproofs R1CS prover on the device (bulletproofs.hip): geometric progressions, the vector polynomials
// l(X) and r(X) of bulletproofs/src/arithmetic_circuit.rs:411-531 with their inner products and their evaluation at x, and the
// a / b half of a round of inner_product_proof::prove (:46-102).  The host entries behind zkp_fr_powers_dev /
// zkp_fr_bp_t_coeffs_dev / zkp_fr_bp_lr_eval_dev / zkp_fr_ipa_fold_ab_dev.  Fr only: one object serves both curves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

constexpr uint32_t BP_THREADS = 256;      // threads per workgroup of every pass
// A pass runs T = BP_THREADS * min(ceil(n / BP_THREADS), BP_MAX_GROUPS) threads; thread j owns the indices j, j + T, ...
// (the ownership of zkp_fr_poly_eval_many_dev): a thread owns a second index from n = BP_THREADS * BP_MAX_GROUPS + 1 on.
constexpr uint32_t BP_MAX_GROUPS = 512;
// The nine sums of t_coeffs are reduced over a workgroup BP_SUM_GROUP at a time: 3 * 256 * 32 bytes = 24 KB of LDS, reused.
constexpr uint32_t BP_SUM_GROUP = 3;
constexpr int BP_MAX_LOG = 28;            // N, n <= 2^28

// after the NULL checks of capi.hip: every other rule, then the work; each returns when its outputs are written
void fr_powers(zkp_ctx* ctx, int curve, const uint64_t* first_host, const uint64_t* ratio_host, uint64_t* out_dev, size_t n);
void fr_bp_t_coeffs(zkp_ctx* ctx, int curve, const zkp_bp_vectors* vecs, const uint64_t* y_host, const uint64_t* z_host,
                    uint64_t* t_out_host);
void fr_bp_lr_eval(zkp_ctx* ctx, int curve, const zkp_bp_vectors* vecs, const uint64_t* y_host, const uint64_t* z_host,
                   const uint64_t* x_host, uint64_t* l_x_dev, uint64_t* r_x_dev, uint64_t* t_x_out_host);
void fr_ipa_fold_ab(zkp_ctx* ctx, int curve, uint64_t* a_dev, uint64_t* b_dev, size_t n, const uint64_t* x_host, uint64_t* c_out_host);

}  // namespace zkp
