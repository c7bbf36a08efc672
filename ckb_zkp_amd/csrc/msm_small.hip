// Batched small variable-base MSM (zkp_msm_g*_var_batch_dev): `count` independent MSMs over fresh bases in two launches, whatever
// `count` is.  Compiled once per (curve, group): -DZKP_CFG_CURVE={0,1} -DZKP_CFG_GROUP={1,2}.
//
//   launch 1  one wave per (entry k, window w, slice j of <= `slice` points); the wave owns 2^(c-1) XYZZ buckets in LDS:
//             a. digits: each lane reads whole scalars (coalesced, 32 B), walks the K5 digit iterator (msm_digits.hpp) up to
//                window w and counts the digit in an LDS histogram (zero digits and identity bases go to the sentinel key nb);
//             b. a stable LDS counting sort of the slice by bucket: lanes with equal keys in a round are matched with a
//                ballot per key bit and ranked with a popcount, so the order — and the result's projective form — is deterministic;
//             c. the sorted list is cut into 64 equal chunks, one per lane: runs inside a chunk go straight to their bucket, the
//                first and last run of each chunk go to two boundary slots per lane;
//             d. a level-synchronous segmented tree over the 128 boundary slots (keys ascending) adds each run's pieces into its
//                bucket; a bucket gets at most one addition per level, so no two lanes touch one bucket at a time.  Work per lane
//                is <= ceil(m / 64) additions + 7 levels whatever the digit distribution (all scalars equal, all in {0, 1}, ...);
//             e. sum_b (b + 1) B_b in parallel: lane t folds its g = nb / 64 buckets into a running sum S_t and a weighted sum V_t,
//                then a Hillis-Steele suffix scan of S gives sum_t t g S_t = g sum_{u >= 1} suffix_u; one partial per workgroup.
//   launch 2  one wave per entry: a tree over the slices of every window, lane w doubles its window sum c w times, an LDS tree
//             adds the windows, lane 0 writes the Jacobian result.
// Points live in the unsaturated BkPoint layout (bucket_dev.hpp) and every addition streams its operands from LDS / memory
// (add_mem), so the four groups share one code path.
#include "bucket_dev.hpp"
#include "ec_dev.hpp"
#include "msm_digits.hpp"
#include "msm_small.hpp"

#ifndef ZKP_CFG_CURVE
#error "compile with -DZKP_CFG_CURVE=0|1 -DZKP_CFG_GROUP=1|2"
#endif

namespace zkp {

#if ZKP_CFG_CURVE == 0
using SmFq = Bn254Fq;
using SmFr = Bn254Fr;
#else
using SmFq = Bls381Fq;
using SmFr = Bls381Fr;
#endif
#if ZKP_CFG_GROUP == 1
using SmF = Fp<SmFq>;
#else
using SmF = Fp2<SmFq>;
#endif

#define ZKP_SM_CAT3(a, b, c) a##b##c
#define ZKP_SM_SYM(name, cu, gr) ZKP_SM_CAT3(name, cu, gr)
// the same source is compiled four times: one namespace per configuration
namespace ZKP_SM_SYM(small_c, ZKP_CFG_CURVE, ZKP_CFG_GROUP) {

constexpr uint32_t SLOT_EMPTY = 0xffffu;       // key of a boundary slot that holds nothing (above every bucket index)

template <int BY>
__device__ __forceinline__ bool sm_is_inf(const char* p) {     // zz == 0 (BkPoint identity); zz = bytes [BY/2, 3BY/4)
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p + BY / 2);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < BY / 16; i++) o |= w[i];
  return o == 0;
}
template <int BY>
__device__ __forceinline__ void sm_zero(char* p) {
  uint32_t* w = reinterpret_cast<uint32_t*>(p);
#pragma unroll
  for (int i = 0; i < BY / 4; i++) w[i] = 0;
}
template <class F>
__device__ __forceinline__ void sm_dbl(char* p) {
  if (!sm_is_inf<BkPoint<F>::BYTES>(p)) BkPoint<F>::dbl_mem(p, p);
}
// affine Montgomery point i of the entry (negated for a negative digit) -> BkPoint layout at out
template <class F>
__device__ __forceinline__ void sm_stage(const uint32_t* xy, uint32_t i, bool neg, char* out) {
  Affine<F> a = Affine<F>::load(xy + (size_t)i * (Affine<F>::BYTES / 4));
  if (neg) a.y = a.y.neg();
  BkPoint<F>::from_sat(XYZZ<F>::from_affine(a)).store(out);
}

template <class F, class FrP>
__global__ __launch_bounds__(SMALL_LANES) void small_bucket_kernel(const SmallDesc* __restrict__ descs, uint32_t count,
                                                                   uint32_t slice, int montgomery, char* __restrict__ partial) {
  using B = BkPoint<F>;
  constexpr int BY = B::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint32_t wg = blockIdx.x;
  const int t = threadIdx.x;
  // the entry of this workgroup: the last one whose first workgroup is <= wg (entries without work share first_wg with the next)
  uint32_t lo = 0, hi = count - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (descs[mid].first_wg <= wg) lo = mid;
    else hi = mid - 1;
  }
  const SmallDesc d = descs[lo];
  const uint32_t local = wg - d.first_wg, w = local / d.S, j = local % d.S;
  const int c = (int)d.c;
  const uint32_t nb = 1u << (c - 1);
  const uint32_t p0 = j * slice, m = min(slice, d.n - p0);

  char* bk = smem;                                               // nb buckets
  char* slots = bk + (size_t)nb * BY;                            // 2 boundary slots per lane
  char* stage = slots + SMALL_SLOTS * BY;                        // one staged point per lane
  uint32_t* skey = reinterpret_cast<uint32_t*>(stage + SMALL_LANES * BY);    // SMALL_SLOTS keys
  uint32_t* hist = skey + SMALL_SLOTS;                           // nb + 1 counts -> offsets -> cursors
  uint32_t* srt = hist + nb + 4;                                 // sorted entries: key << 16 | negative << 15 | slice index
  uint16_t* ent = reinterpret_cast<uint16_t*>(srt + slice);      // digit of each slice entry: key | negative << 15

  for (uint32_t q = t; q < nb * (BY / 4); q += SMALL_LANES) reinterpret_cast<uint32_t*>(bk)[q] = 0;
  for (uint32_t q = t; q <= nb; q += SMALL_LANES) hist[q] = 0;
  __syncthreads();

  // a. digits of window w
  for (uint32_t e = t; e < m; e += SMALL_LANES) {
    const uint32_t i = p0 + e;
    uint32_t key = nb, neg = 0;
    if (!(d.inf && d.inf[i])) {
      DigitIter it = load_scalar<FrP>(d.scalars, i, montgomery);
      for (uint32_t v = 0; v <= w; v++) it.next((int)v, c, (int)d.W, nb, key, neg);
      if (key == nb) neg = 0;
    }
    ent[e] = (uint16_t)(key | neg << 15);
    atomicAdd(&hist[key], 1u);
  }
  __syncthreads();
  {                                                              // exclusive scan of the nb + 1 counts
    const uint32_t nk = nb + 1, per = (nk + SMALL_LANES - 1) / SMALL_LANES;
    const uint32_t q0 = min(nk, t * per), q1 = min(nk, q0 + per);
    uint32_t loc = 0;
    for (uint32_t q = q0; q < q1; q++) loc += hist[q];
    uint32_t inc = loc;
    for (int o = 1; o < SMALL_LANES; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)inc, o, SMALL_LANES);
      if (t >= o) inc += y;
    }
    uint32_t run = inc - loc;
    for (uint32_t q = q0; q < q1; q++) {
      const uint32_t h = hist[q];
      hist[q] = run;
      run += h;
    }
  }
  __syncthreads();
  const uint32_t mp = hist[nb];                                  // entries with a non-zero digit: sorted[0, mp)
  __syncthreads();

  // b. stable scatter, 64 entries per round
  for (uint32_t r = 0; r < m; r += SMALL_LANES) {
    const uint32_t e = r + t;
    const bool act = e < m;
    const uint32_t v = act ? ent[e] : 0u;
    const uint32_t key = v & 0x7fffu;
    uint64_t same = __ballot(act);
    for (int b = 0; b < c; b++) {                                // keys are <= nb: c bits
      const bool bit = (key >> b) & 1;
      const uint64_t bb = __ballot(bit);
      same &= bit ? bb : ~bb;
    }
    if (act) {
      const uint32_t rank = (uint32_t)__popcll(same & ((1ull << t) - 1));
      srt[hist[key] + rank] = key << 16 | (v & 0x8000u) | e;
      if ((same >> t) == 1ull) hist[key] += (uint32_t)__popcll(same);   // the highest lane of the group advances the cursor
    }
    __syncthreads();
  }

  // c. one chunk of the sorted list per lane
  {
    const uint32_t L = (mp + SMALL_LANES - 1) / SMALL_LANES;
    const uint32_t s0 = min(mp, t * L), s1 = min(mp, s0 + L);
    char* H = slots + (size_t)(2 * t) * BY;
    char* T = H + BY;                                            // the running sum of the current run
    char* stg = stage + (size_t)t * BY;
    sm_zero<BY>(H);
    sm_zero<BY>(T);
    uint32_t hkey = SLOT_EMPTY, tkey = SLOT_EMPTY;
    if (s0 < s1) {
      uint32_t cur = srt[s0] >> 16;
      bool first = true;
      for (uint32_t q = s0; q < s1; q++) {
        const uint32_t v = srt[q], key = v >> 16;
        if (key != cur) {
          if (first) {
            B::copy_point(H, T);
            hkey = cur;
            first = false;
          } else {
            B::copy_point(bk + (size_t)cur * BY, T);             // a run strictly inside the chunk: this lane owns the bucket
          }
          sm_zero<BY>(T);
          cur = key;
        }
        sm_stage<F>(d.xy, p0 + (v & 0x7fffu), (v & 0x8000u) != 0, stg);
        B::add_mem(T, stg, T);
      }
      tkey = cur;
      if (first) hkey = cur;                                     // one run: H stays the identity under the same key
    }
    skey[2 * t] = hkey;
    skey[2 * t + 1] = tkey;
  }
  __syncthreads();

  // d. boundary runs: the slot at the right end of a block holds the sum of the block's entries with that slot's key
  for (int h = 1; h < SMALL_SLOTS; h <<= 1) {
    if (t < SMALL_SLOTS / (2 * h)) {
      const int i = t * 2 * h + h - 1, k = i + h;
      const uint32_t ki = skey[i], kk = skey[k];
      char* si = slots + (size_t)i * BY;
      if (ki == kk) {
        if (ki != SLOT_EMPTY) B::add_mem(slots + (size_t)k * BY, si, slots + (size_t)k * BY);
      } else {                                                   // ki < kk: block i ends its run
        B::add_mem(bk + (size_t)ki * BY, si, bk + (size_t)ki * BY);
      }
    }
    __syncthreads();
  }
  if (t == 0 && skey[SMALL_SLOTS - 1] != SLOT_EMPTY) {
    char* b = bk + (size_t)skey[SMALL_SLOTS - 1] * BY;
    B::add_mem(b, slots + (size_t)(SMALL_SLOTS - 1) * BY, b);
  }
  __syncthreads();

  // e. sum_b (b + 1) B_b
  const int g = (int)(nb / SMALL_LANES);
  char* R = slots + (size_t)t * BY;
  char* V = slots + (size_t)(SMALL_LANES + t) * BY;
  sm_zero<BY>(R);
  sm_zero<BY>(V);
  for (int b = (t + 1) * g - 1; b >= t * g; b--) {
    B::add_mem(R, bk + (size_t)b * BY, R);
    B::add_mem(V, R, V);                                         // V_t = sum over the group of (b - t g + 1) B_b
  }
  __syncthreads();
  char* X = slots;                                               // S_t, then its suffix sums (double-buffered in the bucket area)
  char* Y = bk;
  for (int h = 1; h < SMALL_LANES; h <<= 1) {
    if (t + h < SMALL_LANES) B::add_mem(X + (size_t)t * BY, X + (size_t)(t + h) * BY, Y + (size_t)t * BY);
    else B::copy_point(Y + (size_t)t * BY, X + (size_t)t * BY);
    __syncthreads();
    char* s = X;
    X = Y;
    Y = s;
  }
  if (t >= 1) {
    char* U = X + (size_t)t * BY;
    for (int s = 1; s < g; s <<= 1) sm_dbl<F>(U);
    B::add_mem(V, U, V);
  }
  __syncthreads();
  for (int h = SMALL_LANES / 2; h > 0; h >>= 1) {
    if (t < h) B::add_mem(V, V + (size_t)h * BY, V);
    __syncthreads();
  }
  if (t == 0) B::copy_point(partial + (size_t)wg * BY, V);
}

template <class F>
__global__ __launch_bounds__(SMALL_LANES) void small_final_kernel(const SmallDesc* __restrict__ descs, char* __restrict__ partial,
                                                                  uint32_t* __restrict__ out_jac) {
  using B = BkPoint<F>;
  constexpr int BY = B::BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const SmallDesc d = descs[blockIdx.x];
  char* base = partial + (size_t)d.first_wg * BY;
  for (uint32_t h = 1; h < d.S; h <<= 1) {                       // slices of each window: pairwise tree, in place
    const uint32_t per = (d.S + 2 * h - 1) / (2 * h);
    for (uint32_t q = t; q < d.W * per; q += SMALL_LANES) {
      const uint32_t w = q / per, jj = (q % per) * 2 * h;
      if (jj + h < d.S) {
        char* a = base + ((size_t)w * d.S + jj) * BY;
        B::add_mem(a, a + (size_t)h * BY, a);
      }
    }
    __syncthreads();
  }
  char* my = smem + (size_t)t * BY;
  if ((uint32_t)t < d.W) {
    B p = B::load(base + (size_t)t * d.S * BY);                  // the chain stays in registers (dbl_mem calls out of line)
    for (uint32_t k = 0; k < (uint32_t)t * d.c; k++) p = p.dbl();  // 2^(c w): the window weight
    p.store(my);
  } else {
    sm_zero<BY>(my);
  }
  __syncthreads();
  for (int h = SMALL_LANES / 2; h > 0; h >>= 1) {
    if (t < h) B::add_mem(my, my + (size_t)h * BY, my);
    __syncthreads();
  }
  if (t == 0) B::load(smem).to_sat().store_jacobian(out_jac + (size_t)blockIdx.x * 3 * F::N);
}

void l_run(hipStream_t s, const SmallDesc* desc, uint32_t count, uint32_t total_wg, uint32_t slice, int montgomery,
           uint32_t lds_bytes, char* partial, uint32_t* out_jac) {
  if (total_wg)
    hipLaunchKernelGGL((small_bucket_kernel<SmF, SmFr>), dim3(total_wg), dim3(SMALL_LANES), lds_bytes, s, desc, count, slice,
                       montgomery, partial);
  if (count)
    hipLaunchKernelGGL((small_final_kernel<SmF>), dim3(count), dim3(SMALL_LANES), SMALL_LANES * BkPoint<SmF>::BYTES, s, desc,
                       partial, out_jac);
}

const MsmSmallVtbl kVtbl = {(size_t)BkPoint<SmF>::BYTES, 3 * SmF::N, l_run};

}  // namespace small_c<curve><group>

const MsmSmallVtbl* ZKP_SM_SYM(msm_small_vtbl_c, ZKP_CFG_CURVE, ZKP_CFG_GROUP)() {
  return &ZKP_SM_SYM(small_c, ZKP_CFG_CURVE, ZKP_CFG_GROUP)::kVtbl;
}

}  // namespace zkp
