// Optimal-ate pairings on the device: zkp_pairing_miller_dev, zkp_pairing_final_exp_dev, zkp_pairing_product_is_one_dev and the
// host-pointer conveniences over them (pairing.hpp; the arithmetic is pairing_dev.hpp).  The primitive behind the Groth16 and KZG10
// verifiers (reference: groth16/src/verifier.rs:8-44, marlin/src/pc/kzg10.rs:158-173): a product of Miller functions per group of
// pairs, then ONE final exponentiation per group.  Compiled once per curve: -DZKP_CFG_CURVE={0,1}, without ZKP_INLINE_MUL.
//
// pr_miller_kernel     one pair per lane, one wave per workgroup.  A pair with a flagged point contributes 1.  The lanes' values go to
//                      LDS (64 Fq12: 24 / 36 KiB) and a segmented suffix product over the wave (6 steps, a lane takes its neighbour
//                      2^s away if that one is in the same group) leaves, in the first lane of every group's part inside the
//                      workgroup, the product of that part.  These heads (lanes at a multiple of 64 or of `group`) write their part to
//                      the partial array; the number of heads below lane i is ceil(i / 64) + ceil(i / group) - ceil(i / lcm), which is
//                      the slot of head i and makes the parts of one group contiguous.  When `group` divides 64 no group spans
//                      workgroups and that slot is the group's index: the heads write the output itself and the second stage and its
//                      scratch are skipped (group 1, the shape of zkp_pairing, and the two pairs of a KZG check among them).
// pr_reduce_kernel     the second stage (only when `group` does not divide 64), one workgroup per group: the lanes stride over the group's parts (one part if the group lies
//                      inside one workgroup, group / 64 + 2 at most), then a tree in LDS; lane 0 writes the group's Miller product.
// pr_final_exp_kernel  one Fq12 per lane; in place allowed.
// pr_is_one_kernel     one byte per Fq12: 1 iff it is the one of GT.
//
// The entries do not test curve or subgroup membership (zkp_g1_subgroup_check / zkp_g2_subgroup_check do).
#include <cstdint>
#include <numeric>

#include "field_dev.hpp"
#include "mem_spans.hpp"
#include "pairing.hpp"

#ifndef ZKP_CFG_CURVE
#error "compile with -DZKP_CFG_CURVE=0|1"
#endif
#ifdef ZKP_INLINE_MUL
#error "pairing.hip is built without ZKP_INLINE_MUL (field_dev.hpp: an inlined multiplier in code this long costs tens of minutes)"
#endif

namespace zkp {

#include "pairing_constants.inc"
}  // namespace zkp
#include "pairing_dev.hpp"
namespace zkp {

#if ZKP_CFG_CURVE == 0
using PrC = Bn254Pairing;
static_assert(PrC::GT_POWER == PAIRING_GT_POWER_BN254, "pairing.hpp and pairing_constants.inc disagree");
#else
using PrC = Bls381Pairing;
static_assert(PrC::GT_POWER == PAIRING_GT_POWER_BLS12_381, "pairing.hpp and pairing_constants.inc disagree");
#endif
using PrF2 = Fp2<PrC::Fq>;
using PrF = Fp<PrC::Fq>;
using Pr = Pairing<PrC, PrF2>;
using PrF12 = Pr::F12;
constexpr int PR_FB = 4 * PrF::N;                 // bytes of an Fq
constexpr int PR_F12B = 12 * PR_FB;               // bytes of an Fq12
static_assert(sizeof(PrF12) == PR_F12B, "an Fq12 is 12 Fq without padding");
static_assert(PAIRING_LANES * PR_F12B <= 64 * 1024, "the wave's Fq12 values fit the static LDS limit");

#define ZKP_PR_CAT(a, b) a##b
#define ZKP_PR_SYM(name, cu) ZKP_PR_CAT(name, cu)
// the same source is compiled twice: one namespace per curve
namespace ZKP_PR_SYM(pairing_c, ZKP_CFG_CURVE) {

__device__ __forceinline__ PrF2 ld2(const char* p) { return PrF2::load(p); }
__device__ __forceinline__ void ld12(PrF12& f, const void* src) {
  const char* p = reinterpret_cast<const char*>(src);
  f.c0.c0 = ld2(p);
  f.c0.c1 = ld2(p + 2 * PR_FB);
  f.c0.c2 = ld2(p + 4 * PR_FB);
  f.c1.c0 = ld2(p + 6 * PR_FB);
  f.c1.c1 = ld2(p + 8 * PR_FB);
  f.c1.c2 = ld2(p + 10 * PR_FB);
}
__device__ __forceinline__ void st12(const PrF12& f, void* dst) {
  char* p = reinterpret_cast<char*>(dst);
  f.c0.c0.store(p);
  f.c0.c1.store(p + 2 * PR_FB);
  f.c0.c2.store(p + 4 * PR_FB);
  f.c1.c0.store(p + 6 * PR_FB);
  f.c1.c1.store(p + 8 * PR_FB);
  f.c1.c2.store(p + 10 * PR_FB);
}

__host__ __device__ __forceinline__ uint64_t cdiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
// heads (lanes at a multiple of PAIRING_LANES or of group) below lane i == the partial slot of head i
__host__ __device__ __forceinline__ uint64_t heads_below(uint64_t i, uint64_t group, uint64_t lcm) {
  return cdiv(i, PAIRING_LANES) + cdiv(i, group) - cdiv(i, lcm);
}

__global__ __launch_bounds__(PAIRING_LANES) void pr_miller_kernel(const uint32_t* g1_xy, const uint8_t* g1_inf, const uint32_t* g2_xy,
                                                                  const uint8_t* g2_inf, uint32_t n, uint32_t group, uint64_t lcm,
                                                                  char* part) {
  __shared__ __attribute__((aligned(16))) char smem[PAIRING_LANES * PR_F12B];
  const int t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * PAIRING_LANES + t;
  const bool act = i < n;
  PrF12 f = Pr::one12();
  if (act && !g1_inf[i] && !g2_inf[i]) {
    const uint32_t* p = g1_xy + i * (2 * PrF::N);
    const char* q = reinterpret_cast<const char*>(g2_xy + i * (4 * PrF::N));
    const PrF px = PrF::load(p), py = PrF::load(p + PrF::N);
    const PrF2 qx = ld2(q), qy = ld2(q + 2 * PR_FB);
    Pr::miller(f, px, py, qx, qy);
  }
  st12(f, smem + t * PR_F12B);
  __syncthreads();
  const uint64_t seg = i / group;
  for (int s = 1; s < PAIRING_LANES; s <<= 1) {
    const bool take = act && t + s < PAIRING_LANES && i + s < n && (i + s) / group == seg;
    PrF12 nb;
    if (take) ld12(nb, smem + (t + s) * PR_F12B);
    __syncthreads();
    if (take) {
      Pr::mul12(f, f, nb);
      st12(f, smem + t * PR_F12B);
    }
    __syncthreads();
  }
  if (act && (t == 0 || i % group == 0)) st12(f, part + heads_below(i, group, lcm) * PR_F12B);
}

__global__ __launch_bounds__(PAIRING_LANES) void pr_reduce_kernel(const char* part, uint32_t group, uint64_t lcm, char* out) {
  __shared__ __attribute__((aligned(16))) char smem[PAIRING_LANES * PR_F12B];
  const int t = threadIdx.x;
  const uint64_t j = blockIdx.x;
  const uint64_t lo = heads_below(j * group, group, lcm), hi = heads_below((j + 1) * group, group, lcm);
  const uint64_t cnt = hi - lo;
  const int live = cnt < PAIRING_LANES ? (int)cnt : PAIRING_LANES;     // lanes that hold a value
  PrF12 f;
  if (t < live) {
    ld12(f, part + (lo + t) * PR_F12B);
    for (uint64_t k = lo + t + PAIRING_LANES; k < hi; k += PAIRING_LANES) {
      PrF12 g;
      ld12(g, part + k * PR_F12B);
      Pr::mul12(f, f, g);
    }
    st12(f, smem + t * PR_F12B);
  }
  __syncthreads();
  for (int h = PAIRING_LANES / 2; h >= 1; h >>= 1) {
    const bool take = t < h && t + h < live;
    if (take) {
      PrF12 g;
      ld12(g, smem + (t + h) * PR_F12B);
      Pr::mul12(f, f, g);
      st12(f, smem + t * PR_F12B);
    }
    __syncthreads();
  }
  if (t == 0) st12(f, out + j * PR_F12B);
}

// out may be in (a lane reads its element before it writes it)
__global__ __launch_bounds__(PAIRING_LANES) void pr_final_exp_kernel(const char* in, uint32_t m, char* out) {
  const uint64_t e = (uint64_t)blockIdx.x * PAIRING_LANES + threadIdx.x;
  if (e >= m) return;
  PrF12 f;
  ld12(f, in + e * PR_F12B);
  Pr::final_exp(f);
  st12(f, out + e * PR_F12B);
}

__global__ void pr_is_one_kernel(const char* gt, uint32_t m, uint8_t* ok) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  PrF12 f;
  ld12(f, gt + e * PR_F12B);
  ok[e] = Pr::is_one12(f) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------- host
void info(uint64_t* out) {
  for (int k = 0; k < 8; k++) out[k] = 0;
  out[0] = PrC::GT_POWER;
  out[1] = PR_F12B / 8;
  out[2] = PAIRING_LANES;
  out[3] = PAIRING_MAX_N;
  out[4] = (uint64_t)PAIRING_LANES * PR_F12B;
}

struct Shape {
  size_t n, group, m;
  uint64_t lcm, parts;       // parts: Fq12 of scratch the two stages need; 0 when one stage is enough
  bool direct;               // group divides PAIRING_LANES: no group spans workgroups, head i has slot i / group == its group
};
Shape shape_of(size_t n, size_t group) {
  ZKP_REQUIRE(n >= 1 && group >= 1 && n <= PAIRING_MAX_N && n % group == 0, ZKP_ERR_BAD_ARG);
  Shape s{n, group, n / group, std::lcm<uint64_t>(group, PAIRING_LANES), 0, false};
  s.direct = s.lcm == PAIRING_LANES;
  s.parts = s.direct ? 0 : heads_below(n, group, s.lcm);
  return s;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
MemSpan span(const void* p, size_t bytes, bool out) { return MemSpan{(uintptr_t)p, (uintptr_t)p + bytes, out}; }

void check_points(const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n, const void* out,
                  size_t out_bytes, bool dev) {
  ZKP_REQUIRE(g1_xy && g1_inf && g2_xy && g2_inf && out, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!dev || (aligned16(g1_xy) && aligned16(g2_xy)), ZKP_ERR_BAD_ARG);     // 16-byte vector loads; host points are staged
  ZKP_REQUIRE(outputs_disjoint({span(g1_xy, n * 2 * PR_FB, false), span(g1_inf, n, false), span(g2_xy, n * 4 * PR_FB, false),
                                span(g2_inf, n, false), span(out, out_bytes, true)}),
              ZKP_ERR_BAD_ARG);
}

// parts: at least s.parts Fq12 of scratch.  A direct shape writes its heads straight to out: one launch, no scratch
void launch_miller(hipStream_t st, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf,
                   const Shape& s, char* parts, char* out) {
  hipLaunchKernelGGL(pr_miller_kernel, dim3((unsigned)cdiv(s.n, PAIRING_LANES)), dim3(PAIRING_LANES), 0, st,
                     reinterpret_cast<const uint32_t*>(g1_xy), g1_inf, reinterpret_cast<const uint32_t*>(g2_xy), g2_inf, (uint32_t)s.n,
                     (uint32_t)s.group, s.lcm, s.direct ? out : parts);
  if (!s.direct)
    hipLaunchKernelGGL(pr_reduce_kernel, dim3((unsigned)s.m), dim3(PAIRING_LANES), 0, st, parts, (uint32_t)s.group, s.lcm, out);
  ZKP_HIP(hipGetLastError());
}
void launch_final_exp(hipStream_t st, const char* in, size_t m, char* out) {
  hipLaunchKernelGGL(pr_final_exp_kernel, dim3((unsigned)cdiv(m, PAIRING_LANES)), dim3(PAIRING_LANES), 0, st, in, (uint32_t)m, out);
  ZKP_HIP(hipGetLastError());
}

void miller(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n,
            size_t group, uint64_t* out_f12) {
  const Shape s = shape_of(n, group);
  ZKP_REQUIRE(aligned16(out_f12), ZKP_ERR_BAD_ARG);
  check_points(g1_xy, g1_inf, g2_xy, g2_inf, n, out_f12, s.m * PR_F12B, true);
  char* parts = ctx->pairing_tmp.as<char>(s.parts * PR_F12B);
  launch_miller(ctx->cur->stream, g1_xy, g1_inf, g2_xy, g2_inf, s, parts, reinterpret_cast<char*>(out_f12));
}

void final_exp(zkp_ctx* ctx, const uint64_t* f12, size_t m, uint64_t* out_gt) {
  ZKP_REQUIRE(f12 && out_gt && m >= 1 && m <= PAIRING_MAX_N, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(aligned16(f12) && aligned16(out_gt), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(same_or_disjoint((uintptr_t)f12, m * PR_F12B, (uintptr_t)out_gt, m * PR_F12B), ZKP_ERR_BAD_ARG);   // in place or apart
  launch_final_exp(ctx->cur->stream, reinterpret_cast<const char*>(f12), m, reinterpret_cast<char*>(out_gt));
}

void product_is_one(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n,
                    size_t group, uint8_t* ok) {
  const Shape s = shape_of(n, group);
  check_points(g1_xy, g1_inf, g2_xy, g2_inf, n, ok, s.m, true);
  char* tmp = ctx->pairing_tmp.as<char>((s.parts + s.m) * PR_F12B);      // the parts, then the m products
  char* gt = tmp + s.parts * PR_F12B;
  hipStream_t st = ctx->cur->stream;
  launch_miller(st, g1_xy, g1_inf, g2_xy, g2_inf, s, tmp, gt);
  launch_final_exp(st, gt, s.m, gt);
  hipLaunchKernelGGL(pr_is_one_kernel, dim3((unsigned)cdiv(s.m, 256)), dim3(256), 0, st, gt, (uint32_t)s.m, ok);
  ZKP_HIP(hipGetLastError());
}

// host points -> the context's staging buffer: g1 | g2 | flags of g1 | flags of g2 | `extra` bytes (16-byte aligned pieces)
struct Staged {
  uint64_t *g1, *g2;
  uint8_t *i1, *i2;
  char* extra;
};
Staged stage(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n,
             size_t extra) {
  const size_t b1 = n * 2 * PR_FB, b2 = n * 4 * PR_FB, bi = (n + 15) / 16 * 16;
  char* base = ctx->pairing_io.as<char>(b1 + b2 + 2 * bi + extra);
  Staged d{reinterpret_cast<uint64_t*>(base), reinterpret_cast<uint64_t*>(base + b1), reinterpret_cast<uint8_t*>(base + b1 + b2),
           reinterpret_cast<uint8_t*>(base + b1 + b2 + bi), base + b1 + b2 + 2 * bi};
  hipStream_t st = ctx->cur->stream;
  ZKP_HIP(hipMemcpyAsync(d.g1, g1_xy, b1, hipMemcpyHostToDevice, st));
  ZKP_HIP(hipMemcpyAsync(d.g2, g2_xy, b2, hipMemcpyHostToDevice, st));
  ZKP_HIP(hipMemcpyAsync(d.i1, g1_inf, n, hipMemcpyHostToDevice, st));
  ZKP_HIP(hipMemcpyAsync(d.i2, g2_inf, n, hipMemcpyHostToDevice, st));
  return d;
}

void pairing_host(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n,
                  uint64_t* gt_out) {
  const Shape s = shape_of(n, 1);
  check_points(g1_xy, g1_inf, g2_xy, g2_inf, n, gt_out, n * PR_F12B, false);
  const Staged d = stage(ctx, g1_xy, g1_inf, g2_xy, g2_inf, n, n * PR_F12B);
  char* parts = ctx->pairing_tmp.as<char>(s.parts * PR_F12B);
  hipStream_t st = ctx->cur->stream;
  launch_miller(st, d.g1, d.i1, d.g2, d.i2, s, parts, d.extra);
  launch_final_exp(st, d.extra, n, d.extra);
  ZKP_HIP(hipMemcpyAsync(gt_out, d.extra, n * PR_F12B, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

void check_host(zkp_ctx* ctx, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy, const uint8_t* g2_inf, size_t n,
                size_t group, uint8_t* ok_out) {
  const Shape s = shape_of(n, group);
  check_points(g1_xy, g1_inf, g2_xy, g2_inf, n, ok_out, s.m, false);
  const Staged d = stage(ctx, g1_xy, g1_inf, g2_xy, g2_inf, n, s.m);
  product_is_one(ctx, d.g1, d.i1, d.g2, d.i2, n, group, reinterpret_cast<uint8_t*>(d.extra));
  hipStream_t st = ctx->cur->stream;
  ZKP_HIP(hipMemcpyAsync(ok_out, d.extra, s.m, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

const PairingVtbl kVtbl = {info, miller, final_exp, product_is_one, pairing_host, check_host};

}  // namespace pairing_c<curve>

const PairingVtbl* ZKP_PR_SYM(pairing_vtbl_c, ZKP_CFG_CURVE)() { return &ZKP_PR_SYM(pairing_c, ZKP_CFG_CURVE)::kVtbl; }

}  // namespace zkp
