// SHA-256 of the reference's gadgets package on the device: the digests (what gadgets/examples/merkle_tree_sha256.rs:16-28 merges
// with), the values of every word whose bits the sha256 gadget allocates (gadgets/src/hashes/sha256.rs:82-249, in the layout of
// sha256.hpp), the complete binary Merkle tree over 32-byte items (gadgets/src/merkletree/cbmt.rs:182-202) and the expansion of
// trace bits into the Fr assignment of a bit circuit.  No field arithmetic, so one object serves both curves.
//
// One lane hashes one message and walks its blocks.  The state and the sixteen-word window of the schedule stay in registers: the 64
// rounds are fully unrolled, so every index into the window is a constant.  The round constants sit in constant memory and are
// indexed by the unrolled round number alone, so they arrive through scalar loads.  The padding is formed in registers.
//
// The kernels:
//   sha256_digest  lane k: the digest of message k, 32 bytes in two 16-byte stores
//   sha256_trace   the same walk; every word of the canonical trace goes to T[w n + k] as it is produced (coalesced over k)
//   sha256_tree    lane = node of one depth: nodes[i] = SHA-256(nodes[2 i + 1] || nodes[2 i + 2]), two compressions
//   bits_expand    lane = (instance, element): the bit a code selects from the trace, as zero or the Montgomery one, 32 bytes
#include "fr_dev.hpp"
#include "sha256.hpp"

namespace zkp {

namespace {

constexpr int NT = (int)SHA256_THREADS;
constexpr int XT = (int)SHA256_EXPAND_THREADS;

// not const: the compiler keeps the table in memory and reads it with scalar loads instead of 64 literals per copy of the rounds
__constant__ uint32_t SHA256_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__device__ __forceinline__ uint32_t rotr(uint32_t x, int by) { return __builtin_rotateright32(x, by); }

__device__ __forceinline__ void iv(uint32_t (&st)[8]) {
  st[0] = 0x6a09e667, st[1] = 0xbb67ae85, st[2] = 0x3c6ef372, st[3] = 0xa54ff53a;
  st[4] = 0x510e527f, st[5] = 0x9b05688c, st[6] = 0x1f83d9ab, st[7] = 0x5be0cd19;
}

// One compression: st <- st + rounds(st, w).  w: the block's sixteen words, then the rolling window of the schedule.  With TRACE,
// word x of the block's record goes to rec[x * n] (sha256.hpp): rec points at the lane's column of the block's first word.
template <bool TRACE>
__device__ __forceinline__ void compress(uint32_t (&st)[8], uint32_t (&w)[16], uint32_t* rec, size_t n) {
  auto put = [&](uint32_t x, uint32_t v) {
    if constexpr (TRACE) rec[(size_t)x * n] = v;
  };
  auto put64 = [&](uint32_t x, uint64_t v) {
    put(x, (uint32_t)v);
    put(x + 1, (uint32_t)(v >> 32));
  };
#pragma unroll
  for (int j = 0; j < 16; j++) put(SHA256_OFF_INPUT + j, w[j]);
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
  uint64_t a_sum = a, e_sum = e;                    // the integers whose low words are a and e
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {
      const uint32_t x15 = w[(i - 15) & 15], x2 = w[(i - 2) & 15];
      const uint32_t t0 = rotr(x15, 7) ^ rotr(x15, 18), s0 = t0 ^ (x15 >> 3);
      const uint32_t t1 = rotr(x2, 17) ^ rotr(x2, 19), s1 = t1 ^ (x2 >> 10);
      const uint64_t sum = (uint64_t)w[i & 15] + s0 + w[(i - 7) & 15] + s1;
      const uint32_t x = SHA256_OFF_SCHED + SHA256_SCHED_WORDS * (i - 16);
      put(x, t0), put(x + 1, s0), put(x + 2, t1), put(x + 3, s1), put64(x + 4, sum);
      w[i & 15] = (uint32_t)sum;
    }
    const uint32_t e1 = rotr(e, 6) ^ rotr(e, 11), S1 = e1 ^ rotr(e, 25), ch = (e & f) ^ (~e & g);
    const uint32_t a1 = rotr(a, 2) ^ rotr(a, 13), S0 = a1 ^ rotr(a, 22), bc = b & c, maj = (a & b) ^ (a & c) ^ bc;
    const uint32_t x = SHA256_OFF_ROUND + SHA256_ROUND_WORDS * i;
    put64(x, e_sum), put(x + 2, e1), put(x + 3, S1), put(x + 4, ch);
    put64(x + 5, a_sum), put(x + 7, a1), put(x + 8, S0), put(x + 9, maj), put(x + 10, bc);
    const uint64_t temp1 = (uint64_t)h + S1 + ch + SHA256_K[i] + w[i & 15];
    e_sum = temp1 + d;
    a_sum = temp1 + S0 + maj;
    h = g, g = f, f = e, e = (uint32_t)e_sum;
    d = c, c = b, b = a, a = (uint32_t)a_sum;
  }
  // a and e are still the deferred operands of round 63: h0 and h4 add the incoming word to the whole sum
  const uint64_t fin[8] = {a_sum + st[0],        (uint64_t)st[1] + b, (uint64_t)st[2] + c, (uint64_t)st[3] + d,
                           e_sum + st[4],        (uint64_t)st[5] + f, (uint64_t)st[6] + g, (uint64_t)st[7] + h};
#pragma unroll
  for (int k = 0; k < 8; k++) {
    put64(SHA256_OFF_FINAL + 2 * k, fin[k]);
    st[k] = (uint32_t)fin[k];
  }
}

// word j of block blk of the padded message m[0, len): the bytes, 0x80, zeros, and in the last block's last two words 8 len
__device__ __forceinline__ uint32_t padded_word(const uint8_t* m, size_t len, bool words, size_t blk, bool last, int j) {
  const size_t o = blk * 64 + 4 * (size_t)j;
  if (o + 4 <= len) {
    if (words) return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(m + o));
    return (uint32_t)m[o] << 24 | (uint32_t)m[o + 1] << 16 | (uint32_t)m[o + 2] << 8 | m[o + 3];
  }
  if (last && j == 14) return (uint32_t)((uint64_t)len >> 29);
  if (last && j == 15) return (uint32_t)((uint64_t)len << 3);
  uint32_t v = 0;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const size_t p = o + t;
    v = v << 8 | (p < len ? m[p] : p == len ? 0x80u : 0u);
  }
  return v;
}

// lane k < n hashes the len bytes at msgs + k len.  TRACE: trace[w n + k] for every w < 1 + SHA256_BLOCK_WORDS blocks; else the
// digest to out + 32 k.  len and blocks are the same in all lanes; a message whose length is a multiple of 4 is read by words
// (msgs is 16-byte aligned).
template <bool TRACE>
__device__ __forceinline__ void hash_message(const uint8_t* __restrict__ msgs, size_t n, size_t len, size_t blocks, size_t k,
                                             uint32_t* __restrict__ trace, uint4* __restrict__ out) {
  const uint8_t* m = msgs + k * len;
  const bool words = (len & 3) == 0;
  uint32_t st[8];
  iv(st);
  if constexpr (TRACE) trace[k] = 0;
#pragma unroll 1
  for (size_t blk = 0; blk < blocks; blk++) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = padded_word(m, len, words, blk, blk + 1 == blocks, j);
    compress<TRACE>(st, w, TRACE ? trace + (1 + (size_t)SHA256_BLOCK_WORDS * blk) * n + k : nullptr, n);
  }
  if constexpr (!TRACE) {
    out[2 * k] = make_uint4(__builtin_bswap32(st[0]), __builtin_bswap32(st[1]), __builtin_bswap32(st[2]), __builtin_bswap32(st[3]));
    out[2 * k + 1] = make_uint4(__builtin_bswap32(st[4]), __builtin_bswap32(st[5]), __builtin_bswap32(st[6]), __builtin_bswap32(st[7]));
  }
}

__global__ __launch_bounds__(NT) void sha256_digest_kernel(const uint8_t* __restrict__ msgs, size_t n, size_t len, size_t blocks,
                                                           uint4* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
  if (k < n) hash_message<false>(msgs, n, len, blocks, k, nullptr, out);
}

__global__ __launch_bounds__(NT) void sha256_trace_kernel(const uint8_t* __restrict__ msgs, size_t n, size_t len, size_t blocks,
                                                          uint32_t* __restrict__ trace) {
  const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
  if (k < n) hash_message<true>(msgs, n, len, blocks, k, trace, nullptr);
}

// lane t < count: node i = lo + t from the 64 bytes of its children at nodes + 32 (2 i + 1); the second block is the padding of
// a 64-byte message.  The children lie past every node of this launch, so nothing read here is written here.
__global__ __launch_bounds__(NT) void sha256_tree_kernel(uint4* nodes, size_t lo, size_t count) {
  const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
  if (t >= count) return;
  const size_t i = lo + t;
  uint32_t st[8], w[16];
  iv(st);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint4 v = nodes[2 * (2 * i + 1) + j];
    w[4 * j] = __builtin_bswap32(v.x), w[4 * j + 1] = __builtin_bswap32(v.y);
    w[4 * j + 2] = __builtin_bswap32(v.z), w[4 * j + 3] = __builtin_bswap32(v.w);
  }
  compress<false>(st, w, nullptr, 0);
#pragma unroll
  for (int j = 0; j < 16; j++) w[j] = j == 0 ? 0x80000000u : j == 15 ? 512u : 0u;
  compress<false>(st, w, nullptr, 0);
  nodes[2 * i] = make_uint4(__builtin_bswap32(st[0]), __builtin_bswap32(st[1]), __builtin_bswap32(st[2]), __builtin_bswap32(st[3]));
  nodes[2 * i + 1] = make_uint4(__builtin_bswap32(st[4]), __builtin_bswap32(st[5]), __builtin_bswap32(st[6]), __builtin_bswap32(st[7]));
}

// One Fr element as a kernel argument, whichever curve it belongs to: 32 bytes on both.  A plain aggregate, so that it stays in the
// kernel argument segment and is read with scalar loads.
struct FrWords {
  uint32_t v[8];
};

// lane (b, j), b < q, j < m: code[j] = v << 6 | bit << 1 | neg selects bit `bit` of word v % W of message v / W of instance b, in
// the trace of q mpi messages; z[b z_stride + j] = that bit ^ neg as zero or `one`.  A v outside the instance's W mpi words reads
// nothing and gives the bare neg.  Knows nothing of SHA-256.
__global__ __launch_bounds__(XT) void bits_expand_kernel(const uint32_t* __restrict__ trace, uint32_t W, uint32_t mpi, size_t q,
                                                         const uint32_t* __restrict__ code, size_t m, uint4* __restrict__ z,
                                                         size_t z_stride, FrWords one) {
  const size_t j = (size_t)blockIdx.x * XT + threadIdx.x;
  if (j >= m) return;
  const uint32_t c = code[j], v = c >> 6, msg = v / W, w = v - msg * W;
  const size_t n = q * mpi;
  for (size_t b = blockIdx.y; b < q; b += gridDim.y) {
    const uint32_t word = msg < mpi ? trace[(size_t)w * n + b * mpi + msg] : 0u;
    const uint32_t mask = 0u - (((word >> ((c >> 1) & 31)) ^ c) & 1);          // all ones: the element is `one`
    uint4* o = z + (b * z_stride + j) * 2;
    o[0] = make_uint4(one.v[0] & mask, one.v[1] & mask, one.v[2] & mask, one.v[3] & mask);
    o[1] = make_uint4(one.v[4] & mask, one.v[5] & mask, one.v[6] & mask, one.v[7] & mask);
  }
}

inline MemSpan byte_span(const void* p, size_t bytes, bool out) { return {(uintptr_t)p, (uintptr_t)p + bytes, out}; }

}  // namespace

void sha256_info(uint64_t info[16]) {
  const uint64_t v[16] = {SHA256_BLOCK_WORDS, SHA256_OFF_INPUT, SHA256_OFF_SCHED, SHA256_SCHED_WORDS, SHA256_OFF_ROUND, SHA256_ROUND_WORDS,
                          SHA256_OFF_FINAL, SHA256_MAX_LOG_LEN, SHA256_MAX_LOG_BYTES, SHA256_MAX_LOG_TRACE_WORDS, SHA256_MAX_LOG_LEAVES,
                          SHA256_MAX_LOG_CODE_WORDS, SHA256_THREADS, SHA256_EXPAND_THREADS, 0, 0};
  for (int i = 0; i < 16; i++) info[i] = v[i];
}

static void require_messages(const void* msgs_dev, size_t n, size_t len) {
  ZKP_REQUIRE(len <= ((size_t)1 << SHA256_MAX_LOG_LEN) && n >= 1 && n <= ((size_t)1 << SHA256_MAX_LOG_BYTES) / (len + 1), ZKP_ERR_BAD_ARG);
  require_aligned16(msgs_dev);
}

void sha256_digests(zkp_ctx* ctx, const uint8_t* msgs_dev, size_t n, size_t len, uint8_t* out_dev) {
  require_messages(msgs_dev, n, len);
  require_aligned16(out_dev);
  require_disjoint_outputs({byte_span(msgs_dev, n * len, false), byte_span(out_dev, n * 32, true)});
  hipLaunchKernelGGL(sha256_digest_kernel, dim3(fr_blocks(n, NT)), dim3(NT), 0, ctx->cur->stream, msgs_dev, n, len,
                     (size_t)sha256_blocks(len), reinterpret_cast<uint4*>(out_dev));
  ZKP_HIP(hipGetLastError());
}

void sha256_trace(zkp_ctx* ctx, const uint8_t* msgs_dev, size_t n, size_t len, uint32_t* trace_dev) {
  require_messages(msgs_dev, n, len);
  require_aligned16(trace_dev);
  const uint64_t W = sha256_trace_words(len);
  ZKP_REQUIRE(n <= ((uint64_t)1 << SHA256_MAX_LOG_TRACE_WORDS) / W, ZKP_ERR_BAD_ARG);
  require_disjoint_outputs({byte_span(msgs_dev, n * len, false), byte_span(trace_dev, (size_t)W * n * 4, true)});
  hipLaunchKernelGGL(sha256_trace_kernel, dim3(fr_blocks(n, NT)), dim3(NT), 0, ctx->cur->stream, msgs_dev, n, len,
                     (size_t)sha256_blocks(len), trace_dev);
  ZKP_HIP(hipGetLastError());
}

void sha256_merkle_tree(zkp_ctx* ctx, uint8_t* nodes_dev, size_t n) {
  ZKP_REQUIRE(n >= 1 && n <= ((size_t)1 << SHA256_MAX_LOG_LEAVES), ZKP_ERR_BAD_ARG);
  require_aligned16(nodes_dev);
  if (n < 2) return;
  const size_t inner = n - 1;
  int top = 0;                                        // the depth of node inner - 1
  while (((size_t)2 << top) <= inner) top++;
  for (int d = top; d >= 0; d--) {
    const size_t lo = ((size_t)1 << d) - 1, full = ((size_t)2 << d) - 1, hi = full < inner ? full : inner;
    hipLaunchKernelGGL(sha256_tree_kernel, dim3(fr_blocks(hi - lo, NT)), dim3(NT), 0, ctx->cur->stream,
                       reinterpret_cast<uint4*>(nodes_dev), lo, hi - lo);
  }
  ZKP_HIP(hipGetLastError());
}

void fr_bits_expand(zkp_ctx* ctx, int curve, const uint32_t* trace_dev, size_t words_per_msg, size_t msgs_per_instance, size_t q,
                    const uint32_t* code_dev, size_t m, uint32_t max_v, uint64_t* z_dev, size_t z_stride) {
  fr_require_curve(curve);
  const size_t code_cap = (size_t)1 << SHA256_MAX_LOG_CODE_WORDS, cap32 = (size_t)1 << 32;
  ZKP_REQUIRE(words_per_msg >= 1 && words_per_msg <= code_cap && msgs_per_instance >= 1 && msgs_per_instance <= code_cap / words_per_msg,
              ZKP_ERR_BAD_ARG);
  const size_t words = words_per_msg * msgs_per_instance;
  ZKP_REQUIRE(max_v < words, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(q >= 1 && m >= 1 && z_stride >= m && z_stride <= cap32 / q && q <= ((size_t)1 << SHA256_MAX_LOG_TRACE_WORDS) / words,
              ZKP_ERR_BAD_ARG);
  require_aligned16(trace_dev);
  require_aligned16(code_dev);
  require_aligned16(z_dev);
  require_disjoint_outputs({byte_span(trace_dev, words * q * 4, false), byte_span(code_dev, m * 4, false),
                            fr_span(z_dev, (q - 1) * z_stride + m, true)});
  const hostf::HostField::E one = hostf::fr_field(curve).one_();
  FrWords one_arg;
  memcpy(one_arg.v, one.data(), sizeof(one_arg));               // the first 8 words of a host element are Fr
  const unsigned rows = (unsigned)(q < 65535 ? q : 65535);
  hipLaunchKernelGGL(bits_expand_kernel, dim3(fr_blocks(m, XT), rows), dim3(XT), 0, ctx->cur->stream, trace_dev, (uint32_t)words_per_msg,
                     (uint32_t)msgs_per_instance, q, code_dev, m, reinterpret_cast<uint4*>(z_dev), z_stride, one_arg);
  ZKP_HIP(hipGetLastError());
}

}  // namespace zkp
