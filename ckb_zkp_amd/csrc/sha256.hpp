// SHA-256 on the device (sha256.hip): digests of n byte messages, the canonical trace of every intermediate word that the
// reference's sha256 gadget allocates bits of (gadgets/src/hashes/sha256.rs:82-249), complete binary Merkle trees with SHA-256 as
// the merge (gadgets/examples/merkle_tree_sha256.rs:16-28) and the expansion of trace bits into an Fr assignment.  The host
// entries behind zkp_sha256_* / zkp_fr_bits_expand_dev.  No field arithmetic: one object serves both curves, and the curve enters
// only as the Montgomery one that the expansion writes.
//
// The canonical trace of n messages of len bytes: uint32 T[w n + k], word w < W = 1 + SHA256_BLOCK_WORDS blocks, message k < n,
// blocks = ceil((len + 9) / 64).  Word 0 is 0.  Block b owns the SHA256_BLOCK_WORDS words from 1 + SHA256_BLOCK_WORDS b:
//   SHA256_OFF_INPUT  + j          j < 16: the block's input word j
//   SHA256_OFF_SCHED  + 6 (i - 16) 16 <= i < 64: rotr7 ^ rotr18 of w[i-15]; that ^ shr3; rotr17 ^ rotr19 of w[i-2]; that ^ shr10;
//                                  w[i-16] + s0 + w[i-7] + s1 as lo, hi
//   SHA256_OFF_ROUND  + 11 i       i < 64: the sum that forms e as lo, hi; rotr6 ^ rotr11 of e; that ^ rotr25; ch; the sum that forms a
//                                  as lo, hi; rotr2 ^ rotr13 of a; that ^ rotr22; maj; b & c.  Round 0: the incoming state words, hi = 0
//   SHA256_OFF_FINAL  + 2 k        k < 8: the sum h_k as lo, hi (h0 and h4 fold the operands that round 63 deferred: 8 and 7 operands)
// Sums are the full integers, not reduced mod 2^32.  ckb_zkp_amd/sha256.py holds the same numbers; zkp_sha256_info reports them.
//
// This header is host code without HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zkp_accel.h"

namespace zkp {

constexpr uint32_t SHA256_BLOCK_WORDS = 1024;
constexpr uint32_t SHA256_OFF_INPUT = 0;
constexpr uint32_t SHA256_OFF_SCHED = 16;
constexpr uint32_t SHA256_SCHED_WORDS = 6;
constexpr uint32_t SHA256_OFF_ROUND = 304;
constexpr uint32_t SHA256_ROUND_WORDS = 11;
constexpr uint32_t SHA256_OFF_FINAL = 1008;
// Workgroup of the one-lane-per-message kernels: one wavefront, as in fr_hash.hpp.
constexpr uint32_t SHA256_THREADS = 64;
constexpr uint32_t SHA256_EXPAND_THREADS = 256;
// Caps (== the header's ZKP_SHA256_MAX_*): a message's bytes, n (len + 1), the words of one trace, the leaves of a tree, and the
// word index v of a witness code (v < 2^26 leaves 6 bits for the bit and the complement flag).
constexpr uint32_t SHA256_MAX_LOG_LEN = 20;
constexpr uint32_t SHA256_MAX_LOG_BYTES = 34;
constexpr uint32_t SHA256_MAX_LOG_TRACE_WORDS = 32;
constexpr uint32_t SHA256_MAX_LOG_LEAVES = 27;
constexpr uint32_t SHA256_MAX_LOG_CODE_WORDS = 26;
static_assert(SHA256_OFF_SCHED == SHA256_OFF_INPUT + 16 && SHA256_OFF_ROUND == SHA256_OFF_SCHED + 48 * SHA256_SCHED_WORDS &&
                  SHA256_OFF_FINAL == SHA256_OFF_ROUND + 64 * SHA256_ROUND_WORDS && SHA256_BLOCK_WORDS == SHA256_OFF_FINAL + 16,
              "the four parts of a block record fill it");
static_assert(SHA256_MAX_LOG_LEN == ZKP_SHA256_MAX_LOG_LEN && SHA256_MAX_LOG_BYTES == ZKP_SHA256_MAX_LOG_BYTES &&
                  SHA256_MAX_LOG_TRACE_WORDS == ZKP_SHA256_MAX_LOG_TRACE_WORDS && SHA256_MAX_LOG_LEAVES == ZKP_SHA256_MAX_LOG_LEAVES &&
                  SHA256_MAX_LOG_CODE_WORDS == ZKP_SHA256_MAX_LOG_CODE_WORDS && SHA256_BLOCK_WORDS == ZKP_SHA256_BLOCK_WORDS,
              "the header quotes the same constants");

inline uint64_t sha256_blocks(uint64_t len) { return (len + 9 + 63) / 64; }
inline uint64_t sha256_trace_words(uint64_t len) { return 1 + (uint64_t)SHA256_BLOCK_WORDS * sha256_blocks(len); }

// after the NULL checks of capi.hip: every other rule, then launches only
void sha256_info(uint64_t info[16]);
void sha256_digests(zkp_ctx* ctx, const uint8_t* msgs_dev, size_t n, size_t len, uint8_t* out_dev);
void sha256_trace(zkp_ctx* ctx, const uint8_t* msgs_dev, size_t n, size_t len, uint32_t* trace_dev);
void sha256_merkle_tree(zkp_ctx* ctx, uint8_t* nodes_dev, size_t n);
void fr_bits_expand(zkp_ctx* ctx, int curve, const uint32_t* trace_dev, size_t words_per_msg, size_t msgs_per_instance, size_t q,
                    const uint32_t* code_dev, size_t m, uint32_t max_v, uint64_t* z_dev, size_t z_stride);

}  // namespace zkp
