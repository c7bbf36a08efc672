// Libra's linear-time GKR on the device (gkr.hip): layer evaluation, the bookkeeping tables of eval_hg / eval_fgu and the fused
// rounds of phase_one_prover / phase_two_prover.  The host entries behind zkp_gkr_layer_* / zkp_fr_gkr_*_dev.  Fr only: one object
// serves both curves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ctx.hpp"

namespace zkp {

constexpr int GKR_MAX_LOG = 28;           // gates per layer <= 2^28, nodes below <= 2^28, table length <= 2^28
// A node's gates are summed by ONE thread while there are at most GKR_LONG of them; a longer segment is cut into chunks of
// GKR_CHUNK entries, one workgroup each (DESIGN.md "Libra GKR layers").
constexpr uint32_t GKR_LONG = 256;
constexpr uint32_t GKR_CHUNK = 4096;

struct GkrLong {
  uint32_t node, first_chunk, n_chunks;
};
struct GkrChunk {
  uint32_t begin, end;                    // entries [begin, end) of the grouped list
};

// the gates grouped by one of their wires: segment `node` is ent[ptr[node] .. ptr[node + 1]), gate order within a segment.
// ent[i] = {gate, other wire | op << 31}
struct GkrSide {
  uint32_t* ptr = nullptr;
  uint2* ent = nullptr;
  GkrLong* longs = nullptr;
  GkrChunk* chunks = nullptr;
  uint32_t n_long = 0, n_chunks = 0, max_fan = 0;
};

}  // namespace zkp

// the wiring of one layer (Layer::mid_layer_new, libra/src/circuit.rs:55-80), resident on one device
struct zkp_gkr_layer {
  int device = 0;
  uint64_t n_gates = 0, n_mul = 0;
  uint32_t log_out = 0, log_in = 0;
  uint2* nat = nullptr;                   // natural order: {left, right | op << 31}
  zkp::GkrSide side[2];                   // by left wire, by right wire
  std::vector<void*> owned;
  ~zkp_gkr_layer();
};

namespace zkp {

// after the NULL checks of capi.hip: every other rule, then the work; each returns when its outputs are written
zkp_gkr_layer* gkr_layer_upload(zkp_ctx* ctx, const uint8_t* op, const uint32_t* left, const uint32_t* right, size_t n_gates,
                                uint32_t log_in);
void gkr_layer_free(zkp_ctx* ctx, zkp_gkr_layer* layer);
void gkr_layer_info(const zkp_gkr_layer* layer, uint64_t info[8]);
void fr_gkr_eval_layer(zkp_ctx* ctx, int curve, const zkp_gkr_layer* layer, const uint64_t* in_dev, uint64_t* out_dev);
void fr_gkr_tables(zkp_ctx* ctx, int curve, const zkp_gkr_layer* layer, int phase, const uint64_t* g_dev, const uint64_t* w_dev,
                   uint64_t* const* out_dev);
void fr_gkr_round(zkp_ctx* ctx, int curve, int phase, uint64_t* const* tables_dev, size_t len, const uint64_t* fu_host,
                  const uint64_t* bind_host, uint64_t* evals_out_host);

}  // namespace zkp
