// Hyrax's data-parallel GKR on the device (hyrax.hip): one layer evaluated over n copies of the circuit and the rounds of the
// first sum-check of ZkSumcheckProof::prover, the one over the copy variables.  The host entries behind
// zkp_fr_gkr_eval_layer_batch_dev / zkp_fr_gkr_dp_round_dev.  Fr only: one object serves both curves.  The wiring is the
// zkp_gkr_layer of gkr.hpp; sum-checks #2 and #3 are the tables and rounds of gkr.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gkr.hpp"

namespace zkp {

constexpr int HYRAX_MAX_LOG = 28;         // log_in + log2 n <= 28 and log_out + log2 n <= 28: a layer over all copies
constexpr uint32_t HYRAX_THREADS = 256;   // columns (copies) per workgroup
// The evaluation walks the layer's by-left-node list in chunks of HYRAX_CHUNK entries: workgroup (c, k) owns columns
// [256 c, 256 c + 256) of entries [32 k, 32 k + 32) (DESIGN.md "Hyrax data-parallel GKR").
constexpr uint32_t HYRAX_CHUNK = 32;
constexpr int HYRAX_MAX_LOG_WG = 20;      // workgroups of one evaluation over h columns: ceil(h / 256) * ceil(n_gates / 32) <= 2^20

// after the NULL checks of capi.hip: every other rule, then the work; each returns when its outputs are written
void fr_gkr_eval_layer_batch(zkp_ctx* ctx, int curve, const zkp_gkr_layer* layer, const uint64_t* in_dev, uint64_t* out_dev, size_t n);
void fr_gkr_dp_round(zkp_ctx* ctx, int curve, const zkp_gkr_layer* layer, uint64_t* v_dev, uint64_t* eq_dev, const uint64_t* w_dev,
                     size_t n, size_t len, const uint64_t* bind_host, uint64_t* evals_out_host, uint64_t* finals_dev);

}  // namespace zkp
