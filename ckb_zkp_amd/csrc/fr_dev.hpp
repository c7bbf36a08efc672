// The helpers that Fr-only units (poly.hip, sumcheck.hip, spark.hip, gkr.hip, plonk.hip, fr_open.hip, hyrax.hip, bulletproofs.hip;
// marlin.hip, which has no kernels, for the host-side rules) share: one Fr element (FrArg) or K of them (FrArgs) as a kernel
// argument, the workgroup sum (fr_block_sum), the sum of every workgroup's partials (fr_sum_partials), the curve dispatch
// (with_fr), the argument rules with the aliasing rule of mem_spans.hpp among them, the carving of one scratch allocation
// (Scratch) and the layout of ctx->poly_consts (PolyConsts).
// Header only: no translation unit, no exported symbol.  A new Fr-only unit starts from here.
#pragma once
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "field_dev.hpp"
#include "host_field.hpp"
#include "mem_spans.hpp"

namespace zkp {

// One Fr element (Montgomery) as a kernel argument: no staging copy, no device constant to keep alive.
template <class F>
struct FrArg {
  uint32_t v[F::N];
  explicit FrArg(const void* host) {                        // 32 host bytes; NULL: zero
    static_assert(F::N * 4 == 32, "Fr is 32 bytes on both curves");
    if (host) memcpy(v, host, 32);
    else memset(v, 0, 32);
  }
  __device__ __forceinline__ F get() const {
    F x;
#pragma unroll
    for (int i = 0; i < F::N; i++) x.v[i] = v[i];
    return x;
  }
};

// K Fr elements (Montgomery) as one kernel argument.  An aggregate: `FrArgs<F, K> c;` leaves unset elements undefined, `c{}` zero.
template <class F, int K>
struct FrArgs {
  uint32_t v[K][F::N];
  void set(int k, const void* host32) { memcpy(v[k], host32, 4 * F::N); }
  void set(int k, const hostf::FrE& e) { set(k, e.data()); }
  __device__ __forceinline__ F get(int k) const {           // k uniform: scalar loads from the kernel argument segment
    F x;
#pragma unroll
    for (int i = 0; i < F::N; i++) x.v[i] = v[k][i];
    return x;
  }
};

// Sums NP values per thread over a workgroup of NT threads (NT: the constant the kernel's __launch_bounds__ names; every
// thread calls).  A thread keeps its running values in registers, publishes them in LDS and adds its partner's: one LDS read
// per step.  The totals are valid in thread 0.  smem: NP * NT * 32 bytes, 16-byte aligned; the last step ends on a barrier, so
// smem can be reused at once.  Field addition is exact: the order of the tree does not change a bit of the result.
template <class F, int NT, int NP>
__device__ __forceinline__ void fr_block_sum(F (&acc)[NP], char* smem) {
  static_assert(NT >= 2 && (NT & (NT - 1)) == 0, "a power-of-two workgroup");
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < NP; p++) acc[p].store(smem + (size_t)(p * NT + t) * 32);
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int p = 0; p < NP; p++) {
        acc[p] = acc[p] + F::load(smem + (size_t)(p * NT + t + s) * 32);
        acc[p].store(smem + (size_t)(p * NT + t) * 32);
      }
    }
    __syncthreads();
  }
}

// out[s] = the sum of the nwg partials of sum s, partial[(s * nwg + g) * 8]: one workgroup of NT threads per sum, after a kernel
// whose workgroups each left one partial per sum through fr_block_sum.  Internal linkage: every unit keeps its own copy.
// gkr_final_kernel (several sums per workgroup, combined with fu) and poly.hip's dot_final_kernel (descriptor-driven) are other
// kernels, not copies of this one.
namespace {
template <class P, int NT>
__global__ __launch_bounds__(NT) void fr_sum_partials_kernel(const uint32_t* __restrict__ partial, uint32_t nwg, uint32_t* __restrict__ out) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[NT * 32];
  F acc[1] = {F::zero()};
  for (uint32_t g = threadIdx.x; g < nwg; g += NT) acc[0] = acc[0] + F::load(partial + ((size_t)blockIdx.x * nwg + g) * 8);
  fr_block_sum<F, NT, 1>(acc, smem);
  if (threadIdx.x == 0) acc[0].store(out + (size_t)blockIdx.x * 8);
}
}  // namespace
template <class P, int NT>
void fr_sum_partials(hipStream_t st, const uint32_t* partial, uint32_t nwg, uint32_t sums, uint32_t* out) {
  hipLaunchKernelGGL((fr_sum_partials_kernel<P, NT>), dim3(sums), dim3(NT), 0, st, partial, nwg, out);
}

// fn(Bn254Fr{}) or fn(Bls381Fr{}): the one place where a curve id becomes an Fr parameter type
template <class Fn>
auto with_fr(int curve, Fn&& fn) {
  if (curve == ZKP_BN254) return fn(Bn254Fr{});
  if (curve == ZKP_BLS12_381) return fn(Bls381Fr{});
  throw StatusError{ZKP_ERR_UNSUPPORTED_CURVE};
}

// ---- argument rules (ZKP_ERR_BAD_ARG; the curve: ZKP_ERR_UNSUPPORTED_CURVE)
inline void fr_require_curve(int curve) { ZKP_REQUIRE(curve == ZKP_BN254 || curve == ZKP_BLS12_381, ZKP_ERR_UNSUPPORTED_CURVE); }
inline bool is_pow2(size_t v) { return v && !(v & (v - 1)); }
inline int log2_ceil(size_t v) {                                // the smallest l with 2^l >= v
  int l = 0;
  while (((size_t)1 << l) < v) l++;
  return l;
}
inline unsigned fr_blocks(size_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }
inline hostf::FrE fr_host_load(const uint64_t* host) {          // 32 host bytes
  hostf::FrE e{};
  memcpy(e.data(), host, 32);
  return e;
}
// `count` Fr elements on the host, each below the modulus (a Montgomery word is any canonical residue)
inline void fr_require_canonical(int curve, const uint64_t* host, size_t count) {
  const hostf::HostField fr = hostf::fr_field(curve);
  for (size_t i = 0; i < count; i++) ZKP_REQUIRE(!fr.geq(reinterpret_cast<const uint32_t*>(host) + 8 * i), ZKP_ERR_BAD_ARG);
}
// Fp::load / store are 16-byte vector accesses
inline void require_aligned16(const void* p) { ZKP_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0, ZKP_ERR_BAD_ARG); }
// outputs overlap nothing; inputs may overlap each other (mem_spans.hpp)
inline void require_disjoint_outputs(std::vector<MemSpan> spans) { ZKP_REQUIRE(outputs_disjoint(std::move(spans)), ZKP_ERR_BAD_ARG); }
// n Fr elements at p, as a span
inline MemSpan fr_span(const void* p, size_t n, bool out) { return {(uintptr_t)p, (uintptr_t)p + n * 32, out}; }

// Carves ONE DevBuf allocation into pieces that each start on a 256-byte boundary: take() every piece first, then resolve().
struct Scratch {
  size_t total = 0;
  char* base = nullptr;
  size_t take(size_t bytes) {
    const size_t off = (total + 255) & ~(size_t)255;
    total = off + bytes;
    return off;
  }
  void resolve(DevBuf& buf) { base = reinterpret_cast<char*>(buf.get(total)); }
  template <class T>
  T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};

// ctx->poly_consts: the Fr constants that poly.hip's kernels read through a pointer, by word offset (8 words per element).
// A new user takes a free slot here, never a bare offset at its call site.
struct PolyConsts {
  static constexpr size_t WORDS = 128;
  static constexpr size_t Z = 0;           // fr_vec_op's k, poly_div_linear's z
  static constexpr size_t DIV_EVAL = 16;   // poly_div_linear's p(z)
  static constexpr size_t VFOLD_ONE = 32;  // poly_vanishing_fold's z = 1
  static constexpr size_t MARLIN = 64;     // marlin_round2_prod / marlin_t3_evals / marlin_h2_numerator: up to 6 elements
  static_assert(MARLIN + 6 * 8 <= WORDS, "the Marlin constants fit");
  static uint32_t* at(zkp_ctx* ctx, size_t slot) { return ctx->poly_consts.as<uint32_t>(WORDS) + slot; }
};

}  // namespace zkp
