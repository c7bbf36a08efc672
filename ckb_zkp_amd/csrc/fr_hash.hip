// Algebraic hashes and the complete binary Merkle tree of the reference's gadgets package: mimc_block (gadgets/src/hashes/mimc.rs:49-62),
// poseidon_block (poseidon.rs:553-585), rescue_block (rescue.rs:337-367), their `*_hash` chains, the auxiliary assignment of the mimc
// gadget (mimc.rs:110-157), build_merkle_tree (gadgets/src/merkletree/cbmt.rs:182-202) and build_proof (:31-72).  Fr only, so one
// object serves both curves.  Every constant is the caller's (zkp_hash_params): no table lives here.
//
// One lane computes one permutation, its state in registers.  The work is bound by the integer multiplier (a Rescue block is some
// 25 000 Fr products, a Poseidon block some 1 600, a MiMC-322 block 644) and touches 64 to 96 bytes of global memory per block, so
// the lanes neither share nor stage anything.  The round index, the addresses of the constants and every digit of Rescue's inverse
// exponent are the same in all lanes: the constants are indexed by the loop counter alone and sit behind __restrict__ pointers, so
// they arrive through scalar loads and occupy no vector register between rounds.
//
// Rescue's inverse S-box x^inv_alpha (a 254-bit exponent) is a square-and-multiply over digits of HASH_RESCUE_WINDOW bits that the
// host cuts once per parameter set (most significant first, leading zero digits dropped): per digit w squarings and, for a digit
// d != 0, one product with x^d from a table of 2^w - 1 powers per state element, picked by wave-uniform selects.
//
// The kernels:
//   hash_lanes    lane k: h = h0[k] (or 0), then h <- block(h, m[k][j]) for j < len.  It is the batched block (h0 = xl, m = xr,
//                 len 1), the `*_hash` chain (h0 = 0) and one depth of the tree (lane = node; the children are two elements apart)
//   merkle_tail   one workgroup: the depths 8 .. 0 of the tree, a barrier between depths
//   mimc_trace    lane k: the 2 rounds + 2 values the mimc gadget allocates for block k
//   rescue_check  one lane, at creation: (x^alpha)^inv_alpha == x
//   merkle_paths  lane k: the siblings above leaf k, a gather without arithmetic
// Every element written is canonical.
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "fr_dev.hpp"
#include "fr_hash.hpp"

// The resident parameters of one hash (include/zkp_accel.h zkp_hash_desc), owned by the context that created them.
struct zkp_hash_params {
  zkp_ctx* ctx = nullptr;
  int curve = 0;
  int32_t kind = 0;
  uint32_t rounds = 0, alpha = 0;
  uint32_t ndigits = 0;          // Rescue: the digits of inv_alpha
  uint64_t products = 0;         // Fr products of one block
  char* dev = nullptr;           // constants | mds | aux (Poseidon: a word per round, full or not; Rescue: a word per digit) | check word
  size_t dev_bytes = 0;
  size_t o_mds = 0, o_aux = 0, o_check = 0;
};

namespace zkp {

namespace {

constexpr int NT = (int)HASH_THREADS;
constexpr int TAIL = (int)HASH_TAIL_NODES;
constexpr int M = (int)HASH_WIDTH;
constexpr int RW = (int)HASH_RESCUE_WINDOW;
constexpr int RT = (1 << RW) - 1;                  // powers x^1 .. x^RT per state element
constexpr uint32_t PATHS_THREADS = 256;
static_assert(M == 3, "the permutations are written for the reference's width");

// What every lane of a launch shares.  consts, mds and aux are read-only for the whole launch and reach the kernels as
// __restrict__ arguments.
struct HashK {
  const uint32_t* consts;
  const uint32_t* mds;
  const uint32_t* aux;
  uint32_t rounds, alpha, ndigits;
};

// a word that is the same in every lane, said so to the compiler: branches on it are scalar
__device__ __forceinline__ uint32_t uniform_word(const uint32_t* p) { return __builtin_amdgcn_readfirstlane(*p); }

template <class F>
__device__ __forceinline__ F pow_alpha(const F& x, uint32_t alpha) {        // alpha: 3, 5 or 7, uniform
  const F x2 = x.sqr();
  if (alpha == 3) return x2 * x;
  const F x4 = x2.sqr();
  if (alpha == 5) return x4 * x;
  return x4 * x2 * x;
}

// s <- mds s (mds row-major)
template <class F>
__device__ __forceinline__ void mds_mix(F (&s)[M], const uint32_t* mds) {
  F t[M];
#pragma unroll
  for (int i = 0; i < M; i++)
    t[i] = F::load(mds + (3 * i) * 8) * s[0] + F::load(mds + (3 * i + 1) * 8) * s[1] + F::load(mds + (3 * i + 2) * 8) * s[2];
#pragma unroll
  for (int i = 0; i < M; i++) s[i] = t[i];
}

// The powers x^1 .. x^RT of one state element.  Every index into the table is a constant of the template expansion, never a loop
// counter, and a pick is a chain of selects limb by limb: the table is split into registers before anything could turn a select
// between its entries into an indexed access, which would move it to scratch memory.
template <class F>
__device__ __forceinline__ F select_fr(bool c, const F& a, const F& b) {             // c uniform
  F m;
#pragma unroll
  for (int i = 0; i < F::N; i++) m.v[i] = c ? a.v[i] : b.v[i];
  return m;
}
template <class F>
struct Powers {
  F p[RT];
  template <int... E>
  __device__ __forceinline__ void fill(const F& x, std::integer_sequence<int, E...>) {
    p[0] = x;
    ((p[E + 1] = p[E] * x), ...);
  }
  template <int... E>
  __device__ __forceinline__ F pick(uint32_t d, std::integer_sequence<int, E...>) const {   // x^d, 1 <= d <= RT, d uniform
    F m = p[0];
    ((m = select_fr(d == (uint32_t)E + 2, p[E + 1], m)), ...);
    return m;
  }
};
using PowerSteps = std::make_integer_sequence<int, RT - 1>;

// s[j] <- s[j]^e for the three state elements at once, e as ndigits >= 1 digits of RW bits, most significant (non-zero) first
template <class F>
__device__ __forceinline__ void pow_digits(F (&s)[M], const uint32_t* digits, uint32_t ndigits) {
  Powers<F> t0, t1, t2;
  t0.fill(s[0], PowerSteps{});
  t1.fill(s[1], PowerSteps{});
  t2.fill(s[2], PowerSteps{});
  const uint32_t d0 = uniform_word(digits);
  s[0] = t0.pick(d0, PowerSteps{});
  s[1] = t1.pick(d0, PowerSteps{});
  s[2] = t2.pick(d0, PowerSteps{});
#pragma unroll 1
  for (uint32_t i = 1; i < ndigits; i++) {
#pragma unroll 1
    for (int b = 0; b < RW; b++) {
#pragma unroll
      for (int j = 0; j < M; j++) s[j] = s[j].sqr();
    }
    const uint32_t d = uniform_word(digits + i);
    if (d) {
      s[0] = s[0] * t0.pick(d, PowerSteps{});
      s[1] = s[1] * t1.pick(d, PowerSteps{});
      s[2] = s[2] * t2.pick(d, PowerSteps{});
    }
  }
}

// mimc_block (mimc.rs:49-62)
template <class F>
__device__ __forceinline__ F mimc_block(const HashK& k, F xl, F xr) {
#pragma unroll 1
  for (uint32_t i = 0; i < k.rounds; i++) {
    const F t = xl + F::load(k.consts + (size_t)i * 8);
    const F nx = t.sqr() * t + xr;
    xr = xl;
    xl = nx;
  }
  return xl;
}

// poseidon_block (poseidon.rs:553-585); aux[i] != 0: round i is full
template <class F>
__device__ __forceinline__ F poseidon_block(const HashK& k, F xl, F xr) {
  F s[M] = {xl, xr, F::zero()};
#pragma unroll 1
  for (uint32_t i = 0; i < k.rounds; i++) {
    const bool full = uniform_word(k.aux + i) != 0;
#pragma unroll
    for (int j = 0; j < M; j++) {
      s[j] = s[j] + F::load(k.consts + ((size_t)i * M + j) * 8);
      if (full || j == M - 1) s[j] = pow_alpha(s[j], k.alpha);
    }
    mds_mix(s, k.mds);
  }
  return s[0];
}

// rescue_block (rescue.rs:337-367)
template <class F>
__device__ __forceinline__ F rescue_block(const HashK& k, F xl, F xr) {
  F s[M] = {xl + F::load(k.consts), xr + F::load(k.consts + 8), F::load(k.consts + 16)};
#pragma unroll 1
  for (uint32_t i = 0; i < 2 * k.rounds; i++) {
    if (i & 1) {
      pow_digits(s, k.aux, k.ndigits);
    } else {
#pragma unroll
      for (int j = 0; j < M; j++) s[j] = pow_alpha(s[j], k.alpha);
    }
    mds_mix(s, k.mds);
#pragma unroll
    for (int j = 0; j < M; j++) s[j] = s[j] + F::load(k.consts + ((size_t)(i + 1) * M + j) * 8);
  }
  return s[0];
}

template <int KIND, class F>
__device__ __forceinline__ F hash_block(const HashK& k, const F& xl, const F& xr) {
  if constexpr (KIND == ZKP_HASH_MIMC) return mimc_block(k, xl, xr);
  else if constexpr (KIND == ZKP_HASH_POSEIDON) return poseidon_block(k, xl, xr);
  else return rescue_block(k, xl, xr);
}

// lane k < n: h = h0[k * h0_stride] (h0 == NULL: 0), then h <- block(h, msg[k * msg_stride + j]) for j < len; out[k] = h and, with
// xl_out, xl_out[k] = h before the last block.  Strides in elements.  out may be h0 or msg when the strides are 1 and len is 1: a
// lane reads its own element before it writes it.
template <class P, int KIND>
__global__ __launch_bounds__(NT) void hash_lanes_kernel(const uint32_t* __restrict__ consts, const uint32_t* __restrict__ mds,
                                                        const uint32_t* __restrict__ aux, uint32_t rounds, uint32_t alpha,
                                                        uint32_t ndigits, const uint32_t* h0, size_t h0_stride, const uint32_t* msg,
                                                        size_t msg_stride, uint32_t len, size_t n, uint32_t* out, uint32_t* xl_out) {
  using F = Fp<P>;
  const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
  if (k >= n) return;
  const HashK hk{consts, mds, aux, rounds, alpha, ndigits};
  F h = h0 ? F::load(h0 + k * h0_stride * 8) : F::zero();
  F before = h;
  const uint32_t* m = msg + k * msg_stride * 8;
#pragma unroll 1
  for (uint32_t j = 0; j < len; j++) {
    before = h;
    h = hash_block<KIND>(hk, h, F::load(m + (size_t)j * 8));
  }
  h.store(out + k * 8);
  if (xl_out) before.store(xl_out + k * 8);
}

// One workgroup of TAIL lanes: the nodes [0, inner), inner <= HASH_TAIL_SPAN, by depth from the deepest to the root; lane t of depth
// d computes node 2^d - 1 + t from its children, which are leaves, nodes of an earlier launch, or nodes of the depth before, behind
// the barrier.  chain != 0: merge(l, r) = block(block(0, l), r), else block(l, r).
template <class P, int KIND>
__global__ __launch_bounds__(TAIL) void merkle_tail_kernel(const uint32_t* __restrict__ consts, const uint32_t* __restrict__ mds,
                                                           const uint32_t* __restrict__ aux, uint32_t rounds, uint32_t alpha,
                                                           uint32_t ndigits, uint32_t* nodes, uint32_t inner, uint32_t chain) {
  using F = Fp<P>;
  const HashK hk{consts, mds, aux, rounds, alpha, ndigits};
  const uint32_t t = threadIdx.x;
  int top = 0;
  while ((2u << top) <= inner) top++;                 // the depth of node inner - 1
  for (int d = top; d >= 0; d--) {
    const uint32_t lo = (1u << d) - 1, full = (2u << d) - 1, hi = full < inner ? full : inner;
    if (t < hi - lo) {
      const size_t i = lo + t;
      const F l = F::load(nodes + (2 * i + 1) * 8), r = F::load(nodes + (2 * i + 2) * 8);
      F h = chain ? F::zero() : l;
#pragma unroll 1
      for (uint32_t j = chain ? 0 : 1; j < 2; j++) h = hash_block<KIND>(hk, h, j == 0 ? l : r);
      h.store(nodes + i * 8);
    }
    __syncthreads();
  }
}

// lane k < n: out + k * stride receives xl, xr, then per round tmp = (xl + c)^2 and the new xl (mimc.rs:110-157)
template <class P>
__global__ __launch_bounds__(NT) void mimc_trace_kernel(const uint32_t* __restrict__ consts, uint32_t rounds, const uint32_t* xl_in,
                                                        const uint32_t* xr_in, size_t n, uint32_t* __restrict__ out, size_t stride) {
  using F = Fp<P>;
  const size_t k = (size_t)blockIdx.x * NT + threadIdx.x;
  if (k >= n) return;
  F xl = F::load(xl_in + k * 8), xr = F::load(xr_in + k * 8);
  uint32_t* o = out + k * stride * 8;
  xl.store(o);
  xr.store(o + 8);
#pragma unroll 1
  for (uint32_t i = 0; i < rounds; i++) {
    const F t = xl + F::load(consts + (size_t)i * 8);
    const F tmp = t.sqr();
    const F nx = tmp * t + xr;
    tmp.store(o + (size_t)(2 + 2 * i) * 8);
    nx.store(o + (size_t)(3 + 2 * i) * 8);
    xr = xl;
    xl = nx;
  }
}

// one lane: *ok = ((x^alpha)^inv_alpha == x) for x = 2, 3 and 5
template <class P>
__global__ __launch_bounds__(NT) void rescue_check_kernel(const uint32_t* __restrict__ digits, uint32_t alpha, uint32_t ndigits, uint32_t* __restrict__ ok) {
  using F = Fp<P>;
  const F two = F::one() + F::one(), three = two + F::one();
  const F x[M] = {two, three, two + three};
  F s[M];
#pragma unroll
  for (int j = 0; j < M; j++) s[j] = pow_alpha(x[j], alpha);
  pow_digits(s, digits, ndigits);
  *ok = (s[0] == x[0] && s[1] == x[1] && s[2] == x[2]) ? 1u : 0u;
}

// lane k < q: the siblings of the nodes from heap index n - 1 + leaf[k] up to a child of the root, then zeros up to stride
// (build_proof, cbmt.rs:31-72); a leaf >= n: ZKP_MERKLE_BAD_LEAF and a zeroed row
__global__ __launch_bounds__(PATHS_THREADS) void merkle_paths_kernel(const uint4* __restrict__ nodes, size_t n,
                                                                     const uint32_t* __restrict__ leaf, size_t q,
                                                                     uint4* __restrict__ out, size_t stride, uint32_t* __restrict__ len) {
  const size_t k = (size_t)blockIdx.x * PATHS_THREADS + threadIdx.x;
  if (k >= q) return;
  const uint32_t li = leaf[k];
  uint4* o = out + k * stride * 2;
  size_t cnt = 0;
  if (li < n) {
    for (size_t i = n - 1 + li; i > 0 && cnt < stride; i = (i - 1) >> 1, cnt++) {
      const size_t sib = ((i + 1) ^ 1) - 1;
      o[2 * cnt] = nodes[2 * sib];
      o[2 * cnt + 1] = nodes[2 * sib + 1];
    }
  }
  len[k] = li < n ? (uint32_t)cnt : ZKP_MERKLE_BAD_LEAF;
  for (; cnt < stride; cnt++) o[2 * cnt] = o[2 * cnt + 1] = make_uint4(0, 0, 0, 0);
}

// ---- host
template <class Fn>
void with_kind(int32_t kind, Fn&& fn) {
  if (kind == ZKP_HASH_MIMC) fn(std::integral_constant<int, ZKP_HASH_MIMC>{});
  else if (kind == ZKP_HASH_POSEIDON) fn(std::integral_constant<int, ZKP_HASH_POSEIDON>{});
  else fn(std::integral_constant<int, ZKP_HASH_RESCUE>{});
}

inline const uint32_t* words(const void* p) { return reinterpret_cast<const uint32_t*>(p); }
inline uint32_t* words(void* p) { return reinterpret_cast<uint32_t*>(p); }
inline const uint32_t* p_consts(const zkp_hash_params* p) { return words(p->dev); }
inline const uint32_t* p_mds(const zkp_hash_params* p) { return words(p->dev + p->o_mds); }
inline const uint32_t* p_aux(const zkp_hash_params* p) { return words(p->dev + p->o_aux); }

void launch_lanes(hipStream_t st, const zkp_hash_params* p, const uint32_t* h0, size_t h0_stride, const uint32_t* msg,
                  size_t msg_stride, uint32_t len, size_t n, uint32_t* out, uint32_t* xl_out) {
  with_fr(p->curve, [&](auto tag) {
    using P = decltype(tag);
    with_kind(p->kind, [&](auto kind) {
      hipLaunchKernelGGL((hash_lanes_kernel<P, decltype(kind)::value>), dim3(fr_blocks(n, NT)), dim3(NT), 0, st, p_consts(p), p_mds(p),
                         p_aux(p), p->rounds, p->alpha, p->ndigits, h0, h0_stride, msg, msg_stride, len, n, out, xl_out);
    });
  });
}

uint32_t alpha_products(uint32_t alpha) { return alpha == 3 ? 2 : alpha == 5 ? 3 : 4; }

void require_params(zkp_ctx* ctx, const zkp_hash_params* p) { ZKP_REQUIRE(p->ctx == ctx, ZKP_ERR_BAD_ARG); }

}  // namespace

void hash_params_create(zkp_ctx* ctx, int curve, const zkp_hash_desc* desc, zkp_hash_params** out) {
  fr_require_curve(curve);
  ZKP_REQUIRE(desc->struct_size >= sizeof(zkp_hash_desc), ZKP_ERR_BAD_ARG);
  const zkp_hash_desc d = *desc;
  ZKP_REQUIRE(d.kind == ZKP_HASH_MIMC || d.kind == ZKP_HASH_POSEIDON || d.kind == ZKP_HASH_RESCUE, ZKP_ERR_BAD_ARG);
  const uint32_t cap = d.kind == ZKP_HASH_MIMC ? HASH_MAX_ROUNDS_MIMC : d.kind == ZKP_HASH_POSEIDON ? HASH_MAX_ROUNDS_POSEIDON
                                                                                                    : HASH_MAX_ROUNDS_RESCUE;
  ZKP_REQUIRE(d.rounds >= 1 && d.rounds <= cap && d.constants, ZKP_ERR_BAD_ARG);
  const bool sponge = d.kind != ZKP_HASH_MIMC;
  if (sponge) ZKP_REQUIRE((d.alpha == 3 || d.alpha == 5 || d.alpha == 7) && d.mds, ZKP_ERR_BAD_ARG);
  if (d.kind == ZKP_HASH_POSEIDON) ZKP_REQUIRE(d.full_round, ZKP_ERR_BAD_ARG);
  const size_t n_consts = d.kind == ZKP_HASH_MIMC ? d.rounds : d.kind == ZKP_HASH_POSEIDON ? (size_t)d.rounds * M : (size_t)(2 * d.rounds + 1) * M;
  fr_require_canonical(curve, d.constants, n_consts);
  if (sponge) fr_require_canonical(curve, d.mds, M * M);

  // the words behind `aux`, and the products of one block by the schedule
  std::vector<uint32_t> aux;
  uint64_t products = 0;
  const uint32_t ap = alpha_products(d.alpha);
  if (d.kind == ZKP_HASH_MIMC) {
    products = 2 * (uint64_t)d.rounds;
  } else if (d.kind == ZKP_HASH_POSEIDON) {
    for (uint32_t i = 0; i < d.rounds; i++) {
      aux.push_back(d.full_round[i] ? 1u : 0u);
      products += (uint64_t)ap * (d.full_round[i] ? M : 1) + M * M;
    }
  } else {
    int top = 255;
    while (top >= 0 && !((d.inv_alpha[top >> 6] >> (top & 63)) & 1)) top--;
    ZKP_REQUIRE(top >= 0, ZKP_ERR_BAD_ARG);
    uint64_t nonzero_after_first = 0;
    for (int dg = top / RW; dg >= 0; dg--) {
      uint32_t v = 0;
      for (int b = RW - 1; b >= 0; b--) {
        const int bit = dg * RW + b;
        v = (v << 1) | (bit < 256 ? (uint32_t)((d.inv_alpha[bit >> 6] >> (bit & 63)) & 1) : 0u);
      }
      if (!aux.empty() && v) nonzero_after_first++;
      aux.push_back(v);
    }
    const uint64_t inv_products = (uint64_t)M * ((RT - 1) + (uint64_t)(aux.size() - 1) * RW + nonzero_after_first);
    products = (uint64_t)d.rounds * ((uint64_t)M * ap + inv_products + 2 * M * M);
  }

  zkp_hash_params* p = new zkp_hash_params();
  p->ctx = ctx;
  p->curve = curve;
  p->kind = d.kind;
  p->rounds = d.rounds;
  p->alpha = sponge ? d.alpha : 0;
  p->ndigits = d.kind == ZKP_HASH_RESCUE ? (uint32_t)aux.size() : 0;
  p->products = products;
  p->o_mds = n_consts * 32;
  p->o_aux = p->o_mds + (sponge ? M * M * 32 : 0);
  p->o_check = p->o_aux + aux.size() * 4;
  p->dev_bytes = p->o_check + 4;
  std::vector<char> host(p->dev_bytes, 0);
  memcpy(host.data(), d.constants, n_consts * 32);
  if (sponge) memcpy(host.data() + p->o_mds, d.mds, M * M * 32);
  if (!aux.empty()) memcpy(host.data() + p->o_aux, aux.data(), aux.size() * 4);
  hipStream_t st = ctx->cur->stream;
  try {
    if (hipMalloc(reinterpret_cast<void**>(&p->dev), p->dev_bytes) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
    ZKP_HIP(hipMemcpyAsync(p->dev, host.data(), p->dev_bytes, hipMemcpyHostToDevice, st));
    uint32_t ok = 1;
    if (d.kind == ZKP_HASH_RESCUE) {
      with_fr(curve, [&](auto tag) {
        hipLaunchKernelGGL(rescue_check_kernel<decltype(tag)>, dim3(1), dim3(1), 0, st, p_aux(p), p->alpha, p->ndigits,
                           words(p->dev + p->o_check));
      });
      ZKP_HIP(hipGetLastError());
      ZKP_HIP(hipMemcpyAsync(&ok, p->dev + p->o_check, 4, hipMemcpyDeviceToHost, st));
    }
    ZKP_HIP(hipStreamSynchronize(st));                            // `host` leaves scope; the check's answer
    ZKP_REQUIRE(ok == 1, ZKP_ERR_BAD_ARG);
  } catch (...) {
    if (p->dev) (void)hipFree(p->dev);
    delete p;
    throw;
  }
  *out = p;
}

void hash_params_free(zkp_ctx* ctx, zkp_hash_params* params) {
  require_params(ctx, params);
  ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));               // a launch in flight still reads the constants
  (void)hipFree(params->dev);
  delete params;
}

void hash_params_info(const zkp_hash_params* params, uint64_t info[8]) {
  info[0] = (uint64_t)params->kind;
  info[1] = (uint64_t)params->curve;
  info[2] = params->rounds;
  info[3] = params->dev_bytes;
  info[4] = params->alpha;
  info[5] = params->products;
  info[6] = info[7] = 0;
}

void fr_hash_blocks(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* xl_dev, const uint64_t* xr_dev, size_t n,
                    uint64_t* out_dev) {
  require_params(ctx, params);
  ZKP_REQUIRE(n >= 1 && n <= ((size_t)1 << HASH_MAX_LOG_BLOCKS), ZKP_ERR_BAD_ARG);
  require_aligned16(xl_dev);
  require_aligned16(xr_dev);
  require_aligned16(out_dev);
  ZKP_REQUIRE(same_or_disjoint((uintptr_t)xl_dev, n * 32, (uintptr_t)out_dev, n * 32) &&
                  same_or_disjoint((uintptr_t)xr_dev, n * 32, (uintptr_t)out_dev, n * 32),
              ZKP_ERR_BAD_ARG);
  launch_lanes(ctx->cur->stream, params, words(xl_dev), 1, words(xr_dev), 1, 1, n, words(out_dev), nullptr);
  ZKP_HIP(hipGetLastError());
}

void fr_hash_chain(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* msgs_dev, size_t n, size_t len, uint64_t* out_dev,
                   uint64_t* xl_out_dev) {
  require_params(ctx, params);
  const size_t cap = (size_t)1 << HASH_MAX_LOG_BLOCKS;
  ZKP_REQUIRE(n >= 1 && len >= 1 && len <= cap && n <= cap / len, ZKP_ERR_BAD_ARG);
  require_aligned16(msgs_dev);
  require_aligned16(out_dev);
  require_aligned16(xl_out_dev);
  require_disjoint_outputs({fr_span(msgs_dev, n * len, false), fr_span(out_dev, n, true), fr_span(xl_out_dev, xl_out_dev ? n : 0, true)});
  launch_lanes(ctx->cur->stream, params, nullptr, 0, words(msgs_dev), len, (uint32_t)len, n, words(out_dev), words(xl_out_dev));
  ZKP_HIP(hipGetLastError());
}

void fr_mimc_trace(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* xl_dev, const uint64_t* xr_dev, size_t n,
                   uint64_t* out_dev, size_t stride) {
  require_params(ctx, params);
  ZKP_REQUIRE(params->kind == ZKP_HASH_MIMC, ZKP_ERR_BAD_ARG);
  const size_t row = 2 * (size_t)params->rounds + 2;
  ZKP_REQUIRE(n >= 1 && n <= ((size_t)1 << HASH_MAX_LOG_BLOCKS) && stride >= row && stride <= ((size_t)1 << 32) / n, ZKP_ERR_BAD_ARG);
  require_aligned16(xl_dev);
  require_aligned16(xr_dev);
  require_aligned16(out_dev);
  require_disjoint_outputs({fr_span(xl_dev, n, false), fr_span(xr_dev, n, false), fr_span(out_dev, (n - 1) * stride + row, true)});
  with_fr(params->curve, [&](auto tag) {
    hipLaunchKernelGGL(mimc_trace_kernel<decltype(tag)>, dim3(fr_blocks(n, NT)), dim3(NT), 0, ctx->cur->stream, p_consts(params),
                       params->rounds, words(xl_dev), words(xr_dev), n, words(out_dev), stride);
  });
  ZKP_HIP(hipGetLastError());
}

void fr_merkle_tree(zkp_ctx* ctx, const zkp_hash_params* params, int32_t merge, uint64_t* nodes_dev, size_t n) {
  require_params(ctx, params);
  ZKP_REQUIRE(merge == ZKP_MERGE_BLOCK || merge == ZKP_MERGE_CHAIN, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(n >= 1 && n <= ((size_t)1 << HASH_MAX_LOG_LEAVES), ZKP_ERR_BAD_ARG);
  require_aligned16(nodes_dev);
  hipStream_t st = ctx->cur->stream;
  uint32_t* nodes = words(nodes_dev);
  const bool chain = merge == ZKP_MERGE_CHAIN;
  for (const MerkleLaunch& l : merkle_plan(n)) {
    if (!l.tail) {
      // node lo + k from the elements 2 lo + 1 + 2 k and 2 lo + 2 + 2 k
      const uint32_t* left = nodes + (2 * l.lo + 1) * 8;
      if (chain) launch_lanes(st, params, nullptr, 0, left, 2, 2, l.hi - l.lo, nodes + l.lo * 8, nullptr);
      else launch_lanes(st, params, left, 2, left + 8, 2, 1, l.hi - l.lo, nodes + l.lo * 8, nullptr);
      continue;
    }
    with_fr(params->curve, [&](auto tag) {
      using P = decltype(tag);
      with_kind(params->kind, [&](auto kind) {
        hipLaunchKernelGGL((merkle_tail_kernel<P, decltype(kind)::value>), dim3(1), dim3(TAIL), 0, st, p_consts(params), p_mds(params),
                           p_aux(params), params->rounds, params->alpha, params->ndigits, nodes, (uint32_t)l.hi, chain ? 1u : 0u);
      });
    });
  }
  ZKP_HIP(hipGetLastError());
}

void fr_merkle_paths(zkp_ctx* ctx, const uint64_t* nodes_dev, size_t n, const uint32_t* leaf_idx_dev, size_t q, uint64_t* out_dev,
                     size_t stride, uint32_t* len_dev) {
  ZKP_REQUIRE(n >= 1 && n <= ((size_t)1 << HASH_MAX_LOG_LEAVES) && q >= 1 && q <= ((size_t)1 << HASH_MAX_LOG_BLOCKS), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(stride >= heap_depth(2 * n - 2) && (stride ? stride : 1) <= ((size_t)1 << 32) / q, ZKP_ERR_BAD_ARG);
  require_aligned16(nodes_dev);
  require_aligned16(out_dev);
  ZKP_REQUIRE(((uintptr_t)leaf_idx_dev & 3) == 0 && ((uintptr_t)len_dev & 3) == 0, ZKP_ERR_BAD_ARG);
  require_disjoint_outputs({fr_span(nodes_dev, 2 * n - 1, false), MemSpan{(uintptr_t)leaf_idx_dev, (uintptr_t)leaf_idx_dev + q * 4, false},
                            fr_span(out_dev, q * stride, true), MemSpan{(uintptr_t)len_dev, (uintptr_t)len_dev + q * 4, true}});
  hipLaunchKernelGGL(merkle_paths_kernel, dim3(fr_blocks(q, PATHS_THREADS)), dim3(PATHS_THREADS), 0, ctx->cur->stream,
                     reinterpret_cast<const uint4*>(nodes_dev), n, leaf_idx_dev, q, reinterpret_cast<uint4*>(out_dev), stride, len_dev);
  ZKP_HIP(hipGetLastError());
}

}  // namespace zkp
