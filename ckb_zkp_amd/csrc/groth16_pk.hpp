// The device-resident Groth16 proving key: what groth16_key.hip builds, describes and frees and what the provers read — the
// single-device prover of groth16.hip and the multi-device prover of groth16_multi.hip — and the steps of a proof that groth16.hip
// (which holds the kernels) lends the multi-device prover.  Private to those three units.
#pragma once
#include <vector>

#include "internal.hpp"

struct DevCsr {
  uint32_t* row_ptr = nullptr;
  uint32_t* col = nullptr;
  uint32_t* coeff = nullptr;
  size_t nnz = 0;
};

struct zkp_groth16_pk {
  int curve = 0;
  uint32_t num_inputs = 0, num_aux = 0, num_constraints = 0;
  int log_n = 0;
  size_t N = 0, nz = 0;
  DevCsr m[3];
  uint64_t hA = 0, hB1 = 0, hB2 = 0, hH = 0, hL = 0;
  bool share_b_sort = false;     // b_g1_query / b_g2_query: same length, window configuration and identity pattern
  bool chain_lh = false;         // H accumulates into L's buckets: one bucket reduction for l' + h_acc (bucket chaining, internal.hpp MsmJob)
  bool share_al_sort = false;    // L (stored index-aligned with z) reuses A's bucket sort: same scalars, same identity pattern
  bool share_l1 = false;         // A, L and (b_in_l1) B2 (+B1) share ONE level-1 sort pass over z (each filters its identities at level 2)
  bool b_in_l1 = false;          // the B queries have A's window configuration and take part in the shared pass
  bool c_folded = false;         // hL holds L - C^T G (fold_c_into_l): the prover skips C z and the c chain of the witness map
  bool h_lagrange = false;       // hH holds the H query in EVALUATION form over the coset (lagrange_h, groth16_key.hip): the prover skips the last transform
  // Base-sharded key (BASELINE configs[4]): this rank holds elements [q_lo, q_lo + q_n) of every
  // (extended) query; world == 0 means the whole key.  Index order: A, B1, B2, H, L.
  int shard_rank = 0, shard_world = 0;
  size_t q_lo[5] = {0, 0, 0, 0, 0}, q_n[5] = {0, 0, 0, 0, 0};
  struct PerLane {   // per in-flight proof (zkp_ctx lanes)
    zkp::DevBuf abc;      // 3 * N Fr
    zkp::DevBuf S;        // nz + 4 Fr
    zkp::DevBuf results;  // 6 XYZZ (G2-sized slots)
    zkp::DevBuf proof;    // [r, s] + device proof + flags
    // hipGraph of one proof on this lane (ZKP_GRAPH=1): state 0 = never run, 1 = ran eagerly once (scratch allocated,
    // signature recorded), 2 = captured.  `sig` = every device pointer the captured launches embed.
    int warmed = 0;        // > 0: a group of that many fused proofs (1 = a single proof) has run on this lane with this key: every scratch buffer has its size
    int graph_state = 0;
    hipGraphExec_t graph_exec = nullptr;
    hipGraph_t graph = nullptr;
    std::vector<const void*> sig;
  } lane[zkp_ctx::N_LANES];
  zkp::DevBuf consts;     // zinv etc.
  uint64_t fused_groups = 0;   // fused proof groups the batches of this key have run, warm-up groups left out (zkp_groth16_pk_info)
};

namespace zkp {

// While one lives on a thread, the key uploads of that thread keep the transformed H query and the bases of the C part (the two
// caches of groth16_key.hip) from one upload to the next: the devices of an in-process multi-GPU key are uploaded one after the
// other from the same descriptor, and one transform serves all.  Its end drops both.
struct KeepLagrange {
  KeepLagrange();
  ~KeepLagrange();
  KeepLagrange(const KeepLagrange&) = delete;
  KeepLagrange& operator=(const KeepLagrange&) = delete;
};

// groth16.hip: the steps of one proof on a lane (comments at the definitions).  The witness map on ctx's current stream, as chain
// k -> region k of an abc region and (a, b, c) -> h:
void witness_eval(zkp_ctx* ctx, const zkp_groth16_pk* pk, const uint32_t* z_dev, int k, uint32_t* out);
void witness_transform(zkp_ctx* ctx, const zkp_groth16_pk* pk, uint32_t* buf);
uint32_t* witness_finish(zkp_ctx* ctx, zkp_groth16_pk* pk, uint32_t* a, bool coeffs);
// the three composed: the whole map of proof g of a group of G in the g-th abc region of the current lane
uint32_t* witness_map_dev(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint32_t* z_dev, bool coeffs = true, int g = 0, int G = 1);
// the inputs of a proof, the request of one of its five MSMs, the fork and the join of its lane's streams
void proof_copy_inputs(hipStream_t st, const zkp_groth16_pk* pk, const uint64_t* z, bool z_on_device, const uint64_t* r,
                       const uint64_t* s, uint32_t* S, uint32_t* rs);
void proof_scalar_tails(hipStream_t st, const zkp_groth16_pk* pk, uint32_t* S, const uint32_t* rs, int G);
MsmJob proof_query_job(const zkp_groth16_pk* pk, int idx, const uint32_t* scalars, char* res, size_t slot);
void lane_fork(zkp_lane* lane);
void lane_join(zkp_lane* lane);

}  // namespace zkp
