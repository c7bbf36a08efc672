// Algebraic hashes and the complete binary Merkle tree of the reference's gadgets package (gadgets/src/hashes/{mimc,poseidon,
// rescue}.rs, gadgets/src/merkletree/cbmt.rs) on the device (fr_hash.hip): resident hash parameters, batched permutations with one
// lane per block, the MiMC gadget's auxiliary assignment, the tree and its membership paths.  The host entries behind
// zkp_hash_params_* / zkp_fr_hash_* / zkp_fr_mimc_trace_dev / zkp_fr_merkle_*_dev.  Fr only: one object serves both curves.
// Every constant is the caller's: the unit ships no table.
//
// This header is host code without HIP: tests/c/merkle_plan.cpp includes it alone and prints the launch plan of the tree.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/zkp_accel.h"

namespace zkp {

// The reference's state width M: rate 2 (xl, xr), capacity 1.
constexpr uint32_t HASH_WIDTH = 3;
// Workgroup of the one-lane-per-block kernels: one wavefront, so that 2^10 blocks already spread over 16 compute units.
constexpr uint32_t HASH_THREADS = 64;
// The tail of the tree: one workgroup of this many lanes computes the depths HASH_TAIL_DEPTHS - 1 .. 0, nodes [0, HASH_TAIL_SPAN).
constexpr uint32_t HASH_TAIL_NODES = 256;
constexpr uint32_t HASH_TAIL_DEPTHS = 9;
constexpr uint32_t HASH_TAIL_SPAN = 2 * HASH_TAIL_NODES - 1;
// Bits per digit of the wave-uniform square-and-multiply behind Rescue's inverse S-box (2^w - 1 table entries per state element).
constexpr uint32_t HASH_RESCUE_WINDOW = 2;
// Caps (== the header's ZKP_HASH_MAX_*).
constexpr uint32_t HASH_MAX_ROUNDS_MIMC = 512;
constexpr uint32_t HASH_MAX_ROUNDS_POSEIDON = 128;
constexpr uint32_t HASH_MAX_ROUNDS_RESCUE = 64;
constexpr uint32_t HASH_MAX_LOG_BLOCKS = 28;
constexpr uint32_t HASH_MAX_LOG_LEAVES = 27;
static_assert(HASH_MAX_ROUNDS_MIMC == ZKP_HASH_MAX_ROUNDS_MIMC && HASH_MAX_ROUNDS_POSEIDON == ZKP_HASH_MAX_ROUNDS_POSEIDON &&
              HASH_MAX_ROUNDS_RESCUE == ZKP_HASH_MAX_ROUNDS_RESCUE && HASH_MAX_LOG_BLOCKS == ZKP_HASH_MAX_LOG_BLOCKS &&
              HASH_MAX_LOG_LEAVES == ZKP_HASH_MAX_LOG_LEAVES && HASH_WIDTH == ZKP_HASH_WIDTH, "the header quotes the same constants");
static_assert(HASH_TAIL_NODES == (1u << (HASH_TAIL_DEPTHS - 1)), "the widest depth of the tail fills its workgroup");

// depth of heap index i: floor(log2(i + 1))
inline uint32_t heap_depth(uint64_t i) {
  uint32_t d = 0;
  while (((uint64_t)2 << d) <= i + 1) d++;
  return d;
}

// One launch of zkp_fr_merkle_tree_dev: the nodes [lo, hi), one lane per node (tail: the one workgroup that walks the depths
// HASH_TAIL_DEPTHS - 1 .. 0 with a barrier between them).
struct MerkleLaunch {
  uint64_t lo, hi;
  bool tail;
};

// n leaves at [n - 1, 2 n - 1); inner nodes [0, n - 1), node i from its children 2 i + 1 and 2 i + 2 (cbmt.rs:182-202).
// With D = heap_depth(n - 2), the deepest inner node's depth: one launch per depth D, ..., HASH_TAIL_DEPTHS, then the tail:
// max(0, D - (HASH_TAIL_DEPTHS - 1)) + 1 launches, none for n == 1.  A node's children are one depth below: leaves, or nodes of
// the launch before (of the depth before, inside the tail).
inline std::vector<MerkleLaunch> merkle_plan(uint64_t n) {
  std::vector<MerkleLaunch> plan;
  if (n < 2) return plan;
  const uint64_t inner = n - 1;
  for (uint32_t d = heap_depth(n - 2); d >= HASH_TAIL_DEPTHS; d--) {
    const uint64_t lo = ((uint64_t)1 << d) - 1, top = ((uint64_t)2 << d) - 1;
    plan.push_back({lo, top < inner ? top : inner, false});
  }
  plan.push_back({0, inner < HASH_TAIL_SPAN ? inner : (uint64_t)HASH_TAIL_SPAN, true});
  return plan;
}

// after the NULL checks of capi.hip: every other rule, then the work
void hash_params_create(zkp_ctx* ctx, int curve, const zkp_hash_desc* desc, zkp_hash_params** out);
void hash_params_free(zkp_ctx* ctx, zkp_hash_params* params);
void hash_params_info(const zkp_hash_params* params, uint64_t info[8]);
// launches only, like fr_vec_op
void fr_hash_blocks(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* xl_dev, const uint64_t* xr_dev, size_t n,
                    uint64_t* out_dev);
void fr_hash_chain(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* msgs_dev, size_t n, size_t len, uint64_t* out_dev,
                   uint64_t* xl_out_dev);
void fr_mimc_trace(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* xl_dev, const uint64_t* xr_dev, size_t n,
                   uint64_t* out_dev, size_t stride);
void fr_merkle_tree(zkp_ctx* ctx, const zkp_hash_params* params, int32_t merge, uint64_t* nodes_dev, size_t n);
void fr_merkle_paths(zkp_ctx* ctx, const uint64_t* nodes_dev, size_t n, const uint32_t* leaf_idx_dev, size_t q, uint64_t* out_dev,
                     size_t stride, uint32_t* len_dev);

}  // namespace zkp
