// Transforms over G1 points: zkp_g1_scale_vec_dev (out[i] = [s_i] P_i with one scalar PER LANE, read from device memory) and
// zkp_g1_ntt_dev (the radix-2 transform whose butterflies are (P, Q) -> (P + [w] Q, P - [w] Q) over curve points), the primitive
// behind all-position aSVC proofs (Tomescu et al., "Aggregatable subvector commitments", §3.4, after Feist-Khovratovich) and behind
// turning a coefficient-form KZG key into a Lagrange-form one without the trapdoor.  Compiled once per curve, G1 only:
// -DZKP_CFG_CURVE={0,1}.
//
// One kernel, one lane per scalar multiplication (= per point of scale_vec, per butterfly of a stage), one wave per workgroup:
//   * the lane turns its Montgomery scalar into canonical words (one product by the raw word 1) and recodes them into
//     ND = ceil(256 / W) signed W-bit windows, digits in [-(2^(W-1) - 1), 2^(W-1)], one byte each in its LDS slot; a canonical scalar
//     (< r < 2^255) leaves no carry out of the top window for W = 2, 3, 4;
//   * it builds Q, 2Q, ..., 2^(W-1) Q as BkPoints (unsaturated XYZZ, bucket_dev.hpp) in its LDS slot;
//   * it walks the windows most significant first: W doublings, then one addition of the selected multiple (y negated for a
//     negative digit).  Loop bounds are the same for every lane; a zero digit skips its addition (no second path to serialise).
// The window width is chosen per launch (pick_window): the LDS of a slot bounds the waves of a CU, so a grid that fills the device
// takes narrow windows (more waves per CU) and a small grid, whose time is one wave's latency, takes the widest.
//
// The transform is decimation in time: one launch swaps the points into bit-reversed order in place, stage 0 (twiddle 1) adds and
// subtracts without a multiplication, stage s pairs (j, j + 2^s) with the twiddle w^(k 2^(log_n - 1 - s)), k = j mod 2^s, from a table
// of the n / 2 powers of w (or 1 / w) that one launch builds in the context's scratch.  The inverse ends with one launch that scales
// every point by 1 / n.  Every stage ends in affine form: Montgomery's trick per workgroup over d = ZZ ZZZ of the lane's one or two
// outputs, as the product tree of ipa.hip (one Fermat inversion per workgroup).  So the buffers hold canonical affine points between
// the launches and no projective scratch exists; the tree and the inversion are a few per cent of a stage's multiplications.
// All additions are the complete ones of BkPoint (equal, opposite and identity operands).  Identities are written as
// zkp_fixed_base_mul_g1 writes them: words (0, 0), flag 1.
#include <algorithm>
#include <cstdint>

#include "bucket_dev.hpp"
#include "ec_dev.hpp"
#include "g1_ntt.hpp"

#ifndef ZKP_CFG_CURVE
#error "compile with -DZKP_CFG_CURVE=0|1"
#endif

namespace zkp {

#if ZKP_CFG_CURVE == 0
using GnFq = Bn254Fq;
using GnFr = Bn254Fr;
#else
using GnFq = Bls381Fq;
using GnFr = Bls381Fr;
#endif
using GnF = Fp<GnFq>;
using GnS = Fp<GnFr>;
static_assert(G1N_MAX_LOG <= GnFr::TWO_ADICITY, "the largest transform exceeds the two-adicity");
static_assert(GnS::N == 8, "scalars are eight 32-bit words");

#define ZKP_GN_CAT(a, b) a##b
#define ZKP_GN_SYM(name, cu) ZKP_GN_CAT(name, cu)
// the same source is compiled twice: one namespace per curve
namespace ZKP_GN_SYM(g1_ntt_c, ZKP_CFG_CURVE) {

// LDS of one lane at window width W: the multiples 1 .. 2^(W-1) of Q (BkPoint), then one byte per digit.  W == 0: no multiplication
// (stage 0), only the inversion tree.
template <class F, int W>
struct GnLds {
  static constexpr int FB = 4 * F::N;
  static constexpr int ENT = W ? 1 << (W ? W - 1 : 0) : 0;
  static constexpr int ND = W ? (G1N_SCALAR_BITS + W - 1) / (W ? W : 1) : 0;
  static constexpr int RAW = ENT * BkPoint<F>::BYTES + (ND + 15) / 16 * 16;
  static constexpr int STRIDE = RAW + ((RAW / 16) % 2 ? 0 : 16);    // an odd number of 16-B units: consecutive lanes start on different banks
  static constexpr int TREE = 2 * G1N_LANES * FB;                   // the inversion tree reuses the slots once the tables are dead
  static constexpr int BYTES = G1N_LANES * STRIDE > TREE ? G1N_LANES * STRIDE : TREE;
};

// canonical scalar -> ND signed digits, least significant first; byte = magnitude | 0x80 if negative
template <int W>
__device__ __forceinline__ void gn_recode(const uint32_t (&k)[8], uint8_t* dig) {
  constexpr int ND = (G1N_SCALAR_BITS + W - 1) / W;
  constexpr uint32_t HALF = 1u << (W - 1), MASK = (1u << W) - 1;
  uint32_t carry = 0;
#pragma unroll
  for (int j = 0; j < ND; j++) {
    const int b = j * W, w = b >> 5, o = b & 31;
    uint32_t v = k[w] >> o;
    if (o + W > 32 && w + 1 < 8) v |= k[w + 1] << (32 - o);
    v = (v & MASK) + carry;
    carry = v > HALF ? 1u : 0u;
    dig[j] = (uint8_t)(carry ? ((1u << W) - v) | 0x80u : v);
  }
}

// [k] q with the lane's own digits (see the head of the file); `mine` is the lane's LDS slot
template <class F, int W>
__device__ __forceinline__ BkPoint<F> gn_mul(const Affine<F>& q, const uint32_t (&k)[8], char* mine) {
  using B = BkPoint<F>;
  using T = GnLds<F, W>;
  uint8_t* dig = reinterpret_cast<uint8_t*>(mine + T::ENT * B::BYTES);
  gn_recode<W>(k, dig);
  {
    const B e = B::from_sat(XYZZ<F>::from_affine(q));
    e.store(mine);
    B d = e.dbl();
    d.store(mine + B::BYTES);
    for (int m = 2; m < T::ENT; m++) {
      d.add(e);
      d.store(mine + m * B::BYTES);
    }
  }
  B acc = B::inf();
  for (int j = T::ND - 1; j >= 0; j--) {
    if (j != T::ND - 1)
      for (int b = 0; b < W; b++) acc = acc.dbl();
    const uint32_t c = dig[j], mag = c & 0x7fu;
    if (mag) {
      B op = B::load(mine + (mag - 1) * B::BYTES);
      if (c & 0x80u) op.v.y = ub_neg<4>(op.v.y);
      acc.add(op);
    }
  }
  return acc;
}

// 1 / leaf for every lane of the wave: product tree in LDS, node k at tree + k FB, leaves [G1N_LANES, 2 G1N_LANES); leaf != 0
template <class F>
__device__ __forceinline__ F gn_wave_inverse(const F& leaf, char* tree, int t) {
  constexpr int FB = 4 * F::N;
  leaf.store(tree + (size_t)(G1N_LANES + t) * FB);
  __syncthreads();
  for (int h = G1N_LANES / 2; h >= 1; h >>= 1) {
    if (t < h) {
      const int k = h + t;
      (F::load(tree + (size_t)(2 * k) * FB) * F::load(tree + (size_t)(2 * k + 1) * FB)).store(tree + (size_t)k * FB);
    }
    __syncthreads();
  }
  if (t == 0) F::load(tree + FB).inv().store(tree + FB);
  __syncthreads();
  for (int h = 1; h < G1N_LANES; h <<= 1) {                      // node k holds 1 / (its product): its children get theirs
    if (t < h) {
      const int k = h + t;
      const F ik = F::load(tree + (size_t)k * FB);
      const F a = F::load(tree + (size_t)(2 * k) * FB), b = F::load(tree + (size_t)(2 * k + 1) * FB);
      (ik * b).store(tree + (size_t)(2 * k) * FB);
      (ik * a).store(tree + (size_t)(2 * k + 1) * FB);
    }
    __syncthreads();
  }
  return F::load(tree + (size_t)(G1N_LANES + t) * FB);
}

template <class F>
__device__ __forceinline__ void gn_write(const XYZZ<F>& p, bool id, const F& inv_d, uint32_t* xy, uint8_t* inf, size_t j) {
  uint32_t* o = xy + j * (2 * F::N);
  if (id) {
    Affine<F>::inf().store(o);
    inf[j] = 1;
    return;
  }
  Affine<F>{p.x * (inv_d * p.zzz), p.y * (inv_d * p.zz)}.store(o);   // 1 / ZZ = ZZZ / d, 1 / ZZZ = ZZ / d
  inf[j] = 0;
}

// s < 0: out[i] = [sc[i sc_stride]] in[i], i < lanes (out may equal in: a lane reads index i before it writes index i).
// s >= 0: stage s of the transform in place (out == in): lane i owns the pair (j0, j0 + 2^s), j0 = (i >> s) << (s + 1) | k,
// k = i mod 2^s, twiddle sc[k << tshift]; W == 0 is the stage whose twiddles are all 1.  No pointer here is __restrict__.
template <class F, int W>
__global__ __launch_bounds__(G1N_LANES) void gn_mul_kernel(const uint32_t* in_xy, const uint8_t* in_inf, uint32_t* out_xy,
                                                           uint8_t* out_inf, const uint32_t* sc, uint32_t sc_stride, uint32_t lanes,
                                                           int s, int tshift) {
  using B = BkPoint<F>;
  using T = GnLds<F, W>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * G1N_LANES + t;
  const bool act = i < lanes, pair = s >= 0;
  size_t j0 = 0, j1 = i, si = i * sc_stride;
  if (pair) {
    const size_t k = i & (((size_t)1 << s) - 1);
    j0 = ((i >> s) << (s + 1)) | k;
    j1 = j0 + ((size_t)1 << s);
    si = k << tshift;
  }
  const Affine<F> q = act ? Affine<F>::load(in_xy + j1 * (2 * F::N)) : Affine<F>::inf();
  const bool q_id = !act || (in_inf && in_inf[j1]) || q.is_inf();
  B tq = B::inf();
  if constexpr (W == 0) {
    if (!q_id) tq = B::from_sat(XYZZ<F>::from_affine(q));
  } else {
    if (!q_id) {
      const GnS km = GnS::load(sc + si * 8).from_mont();
      uint32_t k[8];
#pragma unroll
      for (int w = 0; w < 8; w++) k[w] = km.v[w];
      tq = gn_mul<F, W>(q, k, smem + (size_t)t * T::STRIDE);
    }
  }
  B o0 = B::inf(), o1 = tq;
  if (pair) {
    const Affine<F> p = act ? Affine<F>::load(in_xy + j0 * (2 * F::N)) : Affine<F>::inf();
    if (act && !(in_inf && in_inf[j0]) && !p.is_inf()) o0 = B::from_sat(XYZZ<F>::from_affine(p));
    if (!tq.v.inf) o1.v.y = ub_neg<4>(tq.v.y);
    B sum = o0;
    sum.add(tq);                                                   // P + [w] Q
    o0.add(o1);                                                    // P - [w] Q
    o1 = o0;
    o0 = sum;
  }
  const XYZZ<F> p0 = o0.to_sat(), p1 = o1.to_sat();
  const bool id0 = !pair || p0.is_inf(), id1 = !act || p1.is_inf();
  const F d0 = id0 ? F::one() : p0.zz * p0.zzz, d1 = id1 ? F::one() : p1.zz * p1.zzz;
  __syncthreads();                                                 // the tables are dead
  const F e = gn_wave_inverse<F>(d0 * d1, smem, t);                // 1 / (d0 d1)
  if (!act) return;
  if (pair) gn_write<F>(p0, id0, e * d1, out_xy, out_inf, j0);
  gn_write<F>(p1, id1, e * d0, out_xy, out_inf, j1);
}

// points and flags into bit-reversed order, in place: the lane of the smaller index of a pair swaps it
template <class F>
__global__ void gn_bitrev_kernel(uint32_t* xy, uint8_t* inf, uint32_t log_n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> log_n) return;
  const uint32_t r = __brev(i) >> (32 - log_n);
  if (i >= r) return;
  uint32_t* a = xy + (size_t)i * (2 * F::N);
  uint32_t* b = xy + (size_t)r * (2 * F::N);
  const Affine<F> pa = Affine<F>::load(a), pb = Affine<F>::load(b);
  pb.store(a);
  pa.store(b);
  const uint8_t fa = inf[i], fb = inf[r];
  inf[i] = fb;
  inf[r] = fa;
}

// out[i] = w^i (inverse: w^-i) for i < count = n / 2, w the root of zkp_ntt_dev's domain of size n; out[count] = 1 / n
__global__ void gn_twiddle_kernel(uint32_t* out, uint32_t log_n, int inverse, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > count) return;
  if (i == count) {
    GnS n = GnS::zero();
    n.v[log_n / 32] = 1u << (log_n % 32);
    n.to_mont().inv().store(out + (size_t)count * 8);
    return;
  }
  GnS w;
#pragma unroll
  for (int k = 0; k < 8; k++) w.v[k] = inverse ? GnFr::ROOT_INV[k] : GnFr::ROOT[k];
  for (uint32_t k = log_n; k < (uint32_t)GnFr::TWO_ADICITY; k++) w = w.sqr();
  w.pow_u64(i).store(out + (size_t)i * 8);
}

// ------------------------------------------------------------------------------------------- host
bool overlap(const void* a, size_t an, const void* b, size_t bn) {
  if (!a || !b || !an || !bn) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bn && y < x + an;
}

// field products of one multiplication at width W, roughly: 256 doublings and ND + 2^(W-1) - 1 additions
template <int W>
constexpr double mul_cost() {
  return 256 * 9.5 + (GnLds<GnF, W>::ND + GnLds<GnF, W>::ENT - 1) * 13.5;
}
template <int W>
double launch_cost(size_t waves, int cus) {
  const size_t per_cu = std::min<size_t>(4, G1N_LDS_BYTES / GnLds<GnF, W>::BYTES);   // one wave per SIMD is what the model counts
  const size_t slots = per_cu * (size_t)cus;
  return (double)((waves + slots - 1) / slots) * mul_cost<W>();
}
// the width with the fewest products on the critical path: rounds of resident waves x products of one multiplication
int pick_window(zkp_ctx* ctx, size_t lanes) {
#ifdef ZKP_G1N_FORCE_W                                             // A/B builds only (ZKP_BUILD_DEFS_g1_ntt=-DZKP_G1N_FORCE_W=2|3|4)
  return ZKP_G1N_FORCE_W;
#endif
  int cus = 0;
  ZKP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  if (cus < 1) cus = 1;
  const size_t waves = (lanes + G1N_LANES - 1) / G1N_LANES;
  const double c4 = launch_cost<4>(waves, cus), c3 = launch_cost<3>(waves, cus), c2 = launch_cost<2>(waves, cus);
  return c4 <= c3 && c4 <= c2 ? 4 : c3 <= c2 ? 3 : 2;
}

template <int W>
void launch_w(hipStream_t st, const uint32_t* in_xy, const uint8_t* in_inf, uint32_t* out_xy, uint8_t* out_inf, const uint32_t* sc,
              uint32_t sc_stride, size_t lanes, int s, int tshift) {
  using T = GnLds<GnF, W>;
  static_assert(T::BYTES <= G1N_LDS_BYTES, "the window tables of one wave exceed the LDS");
  if (T::BYTES > 64 * 1024)
    ZKP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gn_mul_kernel<GnF, W>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                T::BYTES));
  hipLaunchKernelGGL((gn_mul_kernel<GnF, W>), dim3((unsigned)((lanes + G1N_LANES - 1) / G1N_LANES)), dim3(G1N_LANES), T::BYTES, st,
                     in_xy, in_inf, out_xy, out_inf, sc, sc_stride, (uint32_t)lanes, s, tshift);
  ZKP_HIP(hipGetLastError());
}
void launch(zkp_ctx* ctx, int w, const uint32_t* in_xy, const uint8_t* in_inf, uint32_t* out_xy, uint8_t* out_inf,
            const uint32_t* sc, uint32_t sc_stride, size_t lanes, int s, int tshift) {
  hipStream_t st = ctx->cur->stream;
  switch (w) {
    case 0: return launch_w<0>(st, in_xy, in_inf, out_xy, out_inf, sc, sc_stride, lanes, s, tshift);
    case 2: return launch_w<2>(st, in_xy, in_inf, out_xy, out_inf, sc, sc_stride, lanes, s, tshift);
    case 3: return launch_w<3>(st, in_xy, in_inf, out_xy, out_inf, sc, sc_stride, lanes, s, tshift);
    default: return launch_w<4>(st, in_xy, in_inf, out_xy, out_inf, sc, sc_stride, lanes, s, tshift);
  }
}

void scale_vec(zkp_ctx* ctx, const uint64_t* xy, const uint8_t* inf, const uint64_t* scalars, size_t n, uint64_t* out_xy,
               uint8_t* out_inf) {
  if (n == 0) return;
  ZKP_REQUIRE(n <= ((size_t)1 << 31), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE((((uintptr_t)xy | (uintptr_t)out_xy | (uintptr_t)scalars) & 15) == 0, ZKP_ERR_BAD_ARG);   // 16-B vector loads
  // in place: out_xy == xy, out_inf == inf; any other overlap of an output with anything is refused
  const size_t xb = n * Affine<GnF>::BYTES, sb = n * 32;
  ZKP_REQUIRE(out_xy == xy || !overlap(out_xy, xb, xy, xb), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(out_inf == inf || !overlap(out_inf, n, inf, n), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!overlap(out_xy, xb, out_inf, n) && !overlap(out_xy, xb, inf, n) && !overlap(out_xy, xb, scalars, sb), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!overlap(out_inf, n, xy, xb) && !overlap(out_inf, n, scalars, sb), ZKP_ERR_BAD_ARG);
  launch(ctx, pick_window(ctx, n), reinterpret_cast<const uint32_t*>(xy), inf, reinterpret_cast<uint32_t*>(out_xy), out_inf,
         reinterpret_cast<const uint32_t*>(scalars), 1, n, -1, 0);
}

void ntt(zkp_ctx* ctx, uint64_t* xy, uint8_t* inf, uint32_t log_n, int32_t op) {
  ZKP_REQUIRE(log_n >= 1 && log_n <= (uint32_t)G1N_MAX_LOG, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(op == ZKP_NTT_FFT || op == ZKP_NTT_IFFT, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(((uintptr_t)xy & 15) == 0, ZKP_ERR_BAD_ARG);
  const size_t n = (size_t)1 << log_n, half = n / 2;
  ZKP_REQUIRE(!overlap(xy, n * Affine<GnF>::BYTES, inf, n), ZKP_ERR_BAD_ARG);
  const bool inverse = op == ZKP_NTT_IFFT;
  hipStream_t st = ctx->cur->stream;
  uint32_t* tw = ctx->g1_ntt_tw.as<uint32_t>((half + 1) * 8);
  uint32_t* p = reinterpret_cast<uint32_t*>(xy);
  hipLaunchKernelGGL(gn_twiddle_kernel, dim3((unsigned)((half + 256) / 256)), dim3(256), 0, st, tw, log_n, inverse ? 1 : 0,
                     (uint32_t)half);
  hipLaunchKernelGGL(gn_bitrev_kernel<GnF>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p, inf, log_n);
  ZKP_HIP(hipGetLastError());
  launch(ctx, 0, p, inf, p, inf, tw, 0, half, 0, 0);
  const int w = pick_window(ctx, half);
  for (uint32_t s = 1; s < log_n; s++) launch(ctx, w, p, inf, p, inf, tw, 0, half, (int)s, (int)(log_n - 1 - s));
  if (inverse) launch(ctx, pick_window(ctx, n), p, inf, p, inf, tw + half * 8, 0, n, -1, 0);   // every point by 1 / n
}

const G1NttVtbl kVtbl = {scale_vec, ntt};

}  // namespace g1_ntt_c<curve>

const G1NttVtbl* ZKP_GN_SYM(g1_ntt_vtbl_c, ZKP_CFG_CURVE)() { return &ZKP_GN_SYM(g1_ntt_c, ZKP_CFG_CURVE)::kVtbl; }

}  // namespace zkp
