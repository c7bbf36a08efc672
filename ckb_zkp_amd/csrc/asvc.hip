// aSVC subvector commitments (asvc/src/lib.rs): the quotient of Phi(X) by A_I(X) = prod_{i in I} (X - w^i) in the middle of prove_pos
// (:197-212, a dense long division there) and the weights c_i = 1 / A_I'(w^i) of aggregate_proofs (:425-431).  Fr only, so one object
// serves both curves.
//
// With w_i = w^p_i the floor quotient is q[t] = sum_i c_i S_i[t], S_i[t] = Phi[t+1] + w_i S_i[t+1], S_i[n-1] = 0.  The coefficients
// are cut into segments of L = 2^floor(log2 k) <= k: segment s holds [sL, (s+1)L).  For t in segment s, with d = (s+1)L - 1 - t,
//   S_i[t] = (sum over t < j < (s+1)L of Phi[j] w_i^(j-t-1))  +  w_i^d E_i[s],    E_i[s] = sum_{j >= (s+1)L} Phi[j] w_i^(j-(s+1)L).
// Weighted with c_i and summed over i the first part is sum_j Phi[j] (sum_i c_i w_i^m) with m <= L - 2 <= k - 2, and
// sum_i c_i w_i^m = 0 for m < k - 1 (the partial fractions of X^m / A_I): it cancels exactly.  So
//   q[t] = sum_i (c_i E_i[s]) w_i^d,
// and E_i is a suffix scan over the segment heads h_i[s] = sum_{j < L} Phi[sL + j] w_i^j with the ratio r_i = w_i^L:
//   E_i[s] = h_i[s+1] + r_i E_i[s+1].
//
// The kernel chain (one stream, no kernel waits for another workgroup):
//   setup    w_i, r_i, r_i^CHUNK, r_i^TILE and the table w_i^(SPAN e), e < L / SPAN, each by one pow_u64 from w (w_i^m = w^(p_i m mod n))
//   diff     d_i = prod_{j != i} (w_i - w_j): one workgroup per position, a product tree in LDS
//   inverse  c = 1 / d: poly.hip's batch inversion
//   heads    thread (s, g): Horner over the L coefficients of segment s for the GROUP positions of group g, running values in registers
//   scan     chunk heads, tile scan, top scan, replay (poly.hip's blocking; the replay folds the tile carry in and multiplies by c_i)
//   out      thread: SPAN consecutive t, accumulators in registers; per position one product per coefficient (u <- u w_i)
// Every element written is canonical and field addition is exact, so the blocking does not change a bit of the result.
#include <algorithm>
#include <cstring>
#include <vector>

#include "asvc.hpp"
#include "fr_dev.hpp"
#include "internal.hpp"

namespace zkp {

namespace {

constexpr int NT = (int)ASVC_THREADS;
constexpr int G = (int)ASVC_GROUP;
constexpr int SPAN = (int)ASVC_SPAN;
constexpr int CH = (int)ASVC_CHUNK;
constexpr int LOG_SPAN = 3, LOG_CH = 5, LOG_TILE = 13;
static_assert((1 << LOG_SPAN) == SPAN && (1 << LOG_CH) == CH && (1u << LOG_TILE) == ASVC_TILE, "the shifts of the setup kernel");

// per-position constants, 8 words each
constexpr int TAB_W = 0, TAB_R = 8, TAB_RC = 16, TAB_RT = 24, TAB_WORDS = 32;

// thread (i, e), e < per: pw[i * per + e] = w_i^(SPAN e) (pw != NULL); e == 0 also leaves the constants of position i
template <class P>
__global__ __launch_bounds__(NT) void asvc_setup_kernel(const uint32_t* __restrict__ pos, uint32_t k, FrArg<Fp<P>> root, size_t n,
                                                        uint32_t log_l, uint32_t per, uint32_t* __restrict__ tab,
                                                        uint32_t* __restrict__ pw) {
  using F = Fp<P>;
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (size_t)k * per) return;
  const uint32_t i = (uint32_t)(idx / per), e = (uint32_t)(idx % per);
  const uint64_t p = pos[i], mask = n - 1;                       // p < n <= 2^30: p << (10 + 13) fits
  const F w = root.get();
  if (pw) w.pow_u64((p * ((uint64_t)e << LOG_SPAN)) & mask).store(pw + idx * 8);
  if (e == 0) {
    uint32_t* t = tab + (size_t)i * TAB_WORDS;
    w.pow_u64(p).store(t + TAB_W);
    w.pow_u64((p << log_l) & mask).store(t + TAB_R);
    w.pow_u64((p << (log_l + LOG_CH)) & mask).store(t + TAB_RC);
    w.pow_u64((p << (log_l + LOG_TILE)) & mask).store(t + TAB_RT);
  }
}

// d[i] = prod_{j != i} (w_i - w_j); the empty product (k == 1) is 1
template <class P>
__global__ __launch_bounds__(NT) void asvc_diff_kernel(const uint32_t* __restrict__ tab, uint32_t k, uint32_t* __restrict__ d) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[NT * 32];
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  const F wi = F::load(tab + (size_t)i * TAB_WORDS + TAB_W);
  F acc = F::one();
  for (uint32_t j = t; j < k; j += NT)
    if (j != i) acc = acc * (wi - F::load(tab + (size_t)j * TAB_WORDS + TAB_W));
  acc.store(smem + t * 32);
  __syncthreads();
  for (uint32_t s = NT / 2; s > 0; s >>= 1) {
    if (t < s) {
      acc = acc * F::load(smem + (t + s) * 32);
      acc.store(smem + t * 32);
    }
    __syncthreads();
  }
  if (t == 0) acc.store(d + (size_t)i * 8);
}

// thread (s, g): H[s * k + i] = sum_{j < L} phi[s L + j] w_i^j for the positions i of group g.  The lanes of a wavefront are
// consecutive groups of one segment: a coefficient load is one line for all of them.  A position past k repeats position k - 1.
template <class P>
__global__ __launch_bounds__(NT) void asvc_heads_kernel(const uint32_t* __restrict__ phi, const uint32_t* __restrict__ tab, uint32_t k,
                                                        uint32_t ngrp, size_t nseg, uint32_t log_l, uint32_t* __restrict__ H) {
  using F = Fp<P>;
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= nseg * ngrp) return;
  const size_t s = idx / ngrp;
  const uint32_t i0 = (uint32_t)(idx % ngrp) * G;
  F w[G], acc[G];
#pragma unroll
  for (int c = 0; c < G; c++) w[c] = F::load(tab + (size_t)(i0 + c < k ? i0 + c : k - 1) * TAB_WORDS + TAB_W);
  const uint32_t* p = phi + (s << log_l) * 8;
  const size_t L = (size_t)1 << log_l;
  F x = F::load(p + (L - 1) * 8);
#pragma unroll
  for (int c = 0; c < G; c++) acc[c] = x;
  for (size_t j = L - 1; j-- > 0;) {
    x = F::load(p + j * 8);
#pragma unroll
    for (int c = 0; c < G; c++) acc[c] = acc[c] * w[c] + x;
  }
#pragma unroll
  for (int c = 0; c < G; c++)
    if (i0 + c < k) acc[c].store(H + (s * k + i0 + c) * 8);
}

// thread (c, i): head[c * k + i] = sum over the segments s of chunk c of H[s * k + i] r_i^(s - c CHUNK)
template <class P>
__global__ __launch_bounds__(NT) void asvc_scan_chunk_kernel(const uint32_t* __restrict__ H, const uint32_t* __restrict__ tab, uint32_t k,
                                                             size_t nseg, size_t nch, uint32_t* __restrict__ head) {
  using F = Fp<P>;
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= nch * k) return;
  const size_t c = idx / k, i = idx % k;
  const F r = F::load(tab + i * TAB_WORDS + TAB_R);
  const size_t lo = c * CH, hi = lo + CH < nseg ? lo + CH : nseg;
  F acc = F::zero();
  for (size_t s = hi; s-- > lo;) acc = acc * r + F::load(H + (s * k + i) * 8);
  acc.store(head + idx * 8);
}

// v[t] <- sum_{t' >= t} v[t'] R^(t' - t) over the NT threads of a workgroup (every thread calls); Rd enters as R.
// After the step with distance d a thread holds the terms [t, t + 2d).  smem: NT * 32 bytes, reusable on return.
template <class F>
__device__ __forceinline__ F geo_suffix_scan(F v, F Rd, char* smem) {
  const int t = threadIdx.x;
  for (int d = 1; d < NT; d <<= 1) {
    v.store(smem + t * 32);
    __syncthreads();
    if (t + d < NT) v = v + Rd * F::load(smem + (t + d) * 32);
    __syncthreads();
    Rd = Rd.sqr();
  }
  return v;
}

// workgroup (tile, i): the chunk heads of one tile become their suffix sums within the tile (ratio r^CHUNK); tsum: the tile's total
template <class P>
__global__ __launch_bounds__(NT) void asvc_scan_tile_kernel(uint32_t* __restrict__ head, const uint32_t* __restrict__ tab, uint32_t k,
                                                            size_t nch, uint32_t* __restrict__ tsum) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[NT * 32];
  const size_t tile = blockIdx.x, i = blockIdx.y, c = tile * NT + threadIdx.x;
  F v = c < nch ? F::load(head + (c * k + i) * 8) : F::zero();
  v = geo_suffix_scan<F>(v, F::load(tab + i * TAB_WORDS + TAB_RC), smem);
  if (c < nch) v.store(head + (c * k + i) * 8);
  if (threadIdx.x == 0) v.store(tsum + (tile * k + i) * 8);
}

// workgroup i: the tile totals become their suffix sums over all tiles (ratio r^TILE), NT tiles at a time from the top; the sum
// of everything above enters the scan through the highest element of the window
template <class P>
__global__ __launch_bounds__(NT) void asvc_scan_top_kernel(uint32_t* __restrict__ tsum, const uint32_t* __restrict__ tab, uint32_t k,
                                                           size_t ntile) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[NT * 32];
  const size_t i = blockIdx.x;
  const int t = threadIdx.x;
  const F R = F::load(tab + i * TAB_WORDS + TAB_RT);
  F carry = F::zero();
  for (size_t win = (ntile + NT - 1) / NT; win-- > 0;) {
    const size_t tl = win * NT + t;
    F v = tl < ntile ? F::load(tsum + (tl * k + i) * 8) : F::zero();
    if (t == NT - 1) v = v + R * carry;
    v = geo_suffix_scan<F>(v, R, smem);
    if (tl < ntile) v.store(tsum + (tl * k + i) * 8);
    if (t == 0) v.store(smem);
    __syncthreads();
    carry = F::load(smem);
    __syncthreads();
  }
}

// thread (c, i): walks the segments of chunk c downwards from the suffix sum above the chunk (its tile's part plus r^(CHUNK (NT - t'))
// times the sum of the tiles above) and replaces H[s * k + i] by c_i E_i[s]
template <class P>
__global__ __launch_bounds__(NT) void asvc_scan_replay_kernel(uint32_t* __restrict__ H, const uint32_t* __restrict__ tab,
                                                              const uint32_t* __restrict__ cw, uint32_t k, size_t nseg, size_t nch,
                                                              size_t ntile, const uint32_t* __restrict__ head,
                                                              const uint32_t* __restrict__ tsum) {
  using F = Fp<P>;
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= nch * k) return;
  const size_t c = idx / k, i = idx % k;
  const F r = F::load(tab + i * TAB_WORDS + TAB_R), ci = F::load(cw + i * 8);
  F acc = F::zero();
  if (c + 1 < nch) {
    const size_t c1 = c + 1, tile1 = c1 / NT;
    acc = F::load(head + (c1 * k + i) * 8);
    if (tile1 + 1 < ntile)
      acc = acc + F::load(tab + i * TAB_WORDS + TAB_RC).pow_u64(NT - c1 % NT) * F::load(tsum + ((tile1 + 1) * k + i) * 8);
  }
  const size_t lo = c * CH, hi = lo + CH < nseg ? lo + CH : nseg;
  for (size_t s = hi; s-- > lo;) {
    uint32_t* h = H + (s * k + i) * 8;
    const F x = F::load(h);
    (acc * ci).store(h);
    acc = acc * r + x;
  }
}

// thread: q[t] for the SPAN coefficients t = SPAN * thread + m, accumulated over all positions in registers and written once.
// E[s * k + i] = c_i E_i[s].  BIG (L >= SPAN): the span lies in one segment, u starts as E * w_i^d (d a multiple of SPAN: the pw
// table) and steps by w_i downwards.  Otherwise a span holds SPAN / L whole segments and u restarts as E at each segment's top.
template <class P, bool BIG>
__global__ __launch_bounds__(NT) void asvc_out_kernel(const uint32_t* __restrict__ E, const uint32_t* __restrict__ tab,
                                                      const uint32_t* __restrict__ pw, uint32_t k, size_t n, uint32_t log_l,
                                                      uint32_t* __restrict__ q) {
  using F = Fp<P>;
  const size_t base = ((size_t)blockIdx.x * NT + threadIdx.x) * SPAN, nq = n - k;
  if (base >= nq) return;
  const size_t lmask = ((size_t)1 << log_l) - 1;
  F acc[SPAN];
#pragma unroll
  for (int m = 0; m < SPAN; m++) acc[m] = F::zero();
  for (uint32_t i = 0; i < k; i++) {
    const F w = F::load(tab + (size_t)i * TAB_WORDS + TAB_W);
    F u = F::zero();
    if (BIG) {
      const size_t top = base + SPAN - 1, d = lmask - (top & lmask);
      u = F::load(E + ((top >> log_l) * k + i) * 8) * F::load(pw + (((size_t)i << log_l) + d) / SPAN * 8);
    }
#pragma unroll
    for (int m = SPAN - 1; m >= 0; m--) {
      const size_t t = base + m;
      if (BIG) {
        if (m != SPAN - 1) u = u * w;
      } else if (t < n) {
        if ((t & lmask) == lmask) u = F::load(E + ((t >> log_l) * k + i) * 8);
        else u = u * w;
      }
      acc[m] = acc[m] + u;
    }
  }
#pragma unroll
  for (int m = 0; m < SPAN; m++)
    if (base + m < nq) acc[m].store(q + (base + m) * 8);
}

hostf::FrE domain_root(int curve, uint32_t log_n) {                // zkp_ntt_dev's w for 2^log_n (ntt.hip)
  const hostf::HostField fr = hostf::fr_field(curve);
  hostf::FrE w{};
  if (curve == ZKP_BN254) memcpy(w.data(), hostf::consts::Bn254Fr::ROOT, 32);
  else memcpy(w.data(), hostf::consts::Bls381Fr::ROOT, 32);
  const int adicity = curve == ZKP_BN254 ? hostf::consts::Bn254Fr::TWO_ADICITY : hostf::consts::Bls381Fr::TWO_ADICITY;
  return fr.pow2k(w, adicity - (int)log_n);
}

// the rules both entries share
void require_subset(int curve, uint32_t log_n, const uint32_t* positions_host, size_t k) {
  fr_require_curve(curve);
  ZKP_REQUIRE(log_n >= 1, ZKP_ERR_BAD_ARG);
  const uint32_t adicity = curve == ZKP_BN254 ? hostf::consts::Bn254Fr::TWO_ADICITY : hostf::consts::Bls381Fr::TWO_ADICITY;
  ZKP_REQUIRE(log_n <= std::min(ASVC_MAX_LOG, adicity), ZKP_ERR_DOMAIN_TOO_LARGE);
  const size_t n = (size_t)1 << log_n;
  ZKP_REQUIRE(positions_host && k >= 1 && k <= std::min<size_t>(n, ASVC_MAX_POSITIONS), ZKP_ERR_BAD_ARG);
  std::vector<uint32_t> sorted(positions_host, positions_host + k);
  std::sort(sorted.begin(), sorted.end());
  ZKP_REQUIRE(sorted.back() < n, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), ZKP_ERR_BAD_ARG);   // a repeat: a zero difference
}

struct Plan {
  size_t n, L, nseg, nch, ntile;
  uint32_t k, log_l, per;
  size_t o_pos, o_tab, o_c, o_pw, o_h, o_head, o_tsum;
};

// positions, constants and weights only (quotient == false) or everything the quotient needs
Plan make_plan(Scratch& sc, uint32_t log_n, size_t k, bool quotient) {
  Plan pl{};
  pl.n = (size_t)1 << log_n;
  pl.k = (uint32_t)k;
  if (quotient)
    while (((size_t)2 << pl.log_l) <= k) pl.log_l++;             // L = 2^floor(log2 k) <= k <= n
  pl.L = (size_t)1 << pl.log_l;
  pl.per = (uint32_t)std::max<size_t>(pl.L / SPAN, 1);
  pl.nseg = pl.n / pl.L;
  pl.nch = (pl.nseg + CH - 1) / CH;
  pl.ntile = (pl.nch + NT - 1) / NT;
  pl.o_pos = sc.take(k * 4);
  pl.o_tab = sc.take(k * TAB_WORDS * 4);
  pl.o_c = sc.take(k * 32);
  if (quotient) {
    pl.o_pw = sc.take(k * pl.per * 32);
    pl.o_h = sc.take(pl.nseg * k * 32);
    pl.o_head = sc.take(pl.nch * k * 32);
    pl.o_tsum = sc.take(pl.ntile * k * 32);
  }
  return pl;
}

// setup, diff, inverse: the constants of every position and c at o_c
template <class P>
void launch_weights(zkp_ctx* ctx, int curve, const Scratch& sc, const Plan& pl, uint32_t log_n, const uint32_t* positions_host,
                    bool with_pw) {
  hipStream_t st = ctx->cur->stream;
  uint32_t* pos = sc.at<uint32_t>(pl.o_pos);
  ZKP_HIP(hipMemcpyAsync(pos, positions_host, (size_t)pl.k * 4, hipMemcpyHostToDevice, st));
  const hostf::FrE w = domain_root(curve, log_n);
  const size_t threads = (size_t)pl.k * pl.per;
  hipLaunchKernelGGL(asvc_setup_kernel<P>, dim3(fr_blocks(threads, NT)), dim3(NT), 0, st, (const uint32_t*)pos, pl.k,
                     FrArg<Fp<P>>(w.data()), pl.n, pl.log_l, pl.per, sc.at<uint32_t>(pl.o_tab),
                     with_pw ? sc.at<uint32_t>(pl.o_pw) : (uint32_t*)nullptr);
  hipLaunchKernelGGL(asvc_diff_kernel<P>, dim3(pl.k), dim3(NT), 0, st, (const uint32_t*)sc.at<uint32_t>(pl.o_tab), pl.k,
                     sc.at<uint32_t>(pl.o_c));
  ZKP_HIP(hipGetLastError());
  fr_batch_inverse(ctx, curve, sc.at<uint64_t>(pl.o_c), pl.k);
}

}  // namespace

void asvc_subset_weights(zkp_ctx* ctx, int curve, uint32_t log_n, const uint32_t* positions_host, size_t k, uint64_t* weights_dev,
                         uint64_t* weights_host) {
  require_subset(curve, log_n, positions_host, k);
  ZKP_REQUIRE(weights_dev || weights_host, ZKP_ERR_BAD_ARG);
  require_aligned16(weights_dev);
  hipStream_t st = ctx->cur->stream;
  Scratch sc;
  const Plan pl = make_plan(sc, log_n, k, false);
  sc.resolve(ctx->poly_tmp);
  with_fr(curve, [&](auto tag) { launch_weights<decltype(tag)>(ctx, curve, sc, pl, log_n, positions_host, false); });
  if (weights_dev) ZKP_HIP(hipMemcpyAsync(weights_dev, sc.at<uint64_t>(pl.o_c), k * 32, hipMemcpyDeviceToDevice, st));
  if (weights_host) {
    ZKP_HIP(hipMemcpyAsync(weights_host, sc.at<uint64_t>(pl.o_c), k * 32, hipMemcpyDeviceToHost, st));
    ZKP_HIP(hipStreamSynchronize(st));
  }
}

void asvc_quotient(zkp_ctx* ctx, int curve, const uint64_t* phi_dev, uint32_t log_n, const uint32_t* positions_host, size_t k,
                   uint64_t* q_dev) {
  require_subset(curve, log_n, positions_host, k);
  ZKP_REQUIRE(phi_dev && q_dev, ZKP_ERR_BAD_ARG);
  require_aligned16(phi_dev);
  require_aligned16(q_dev);
  const size_t n = (size_t)1 << log_n;
  require_disjoint_outputs({fr_span(phi_dev, n, false), fr_span(q_dev, n - k, true)});
  if (k == n) return;                                             // the quotient of a polynomial of degree < n by one of degree n
  hipStream_t st = ctx->cur->stream;
  Scratch sc;
  const Plan pl = make_plan(sc, log_n, k, true);
  sc.resolve(ctx->poly_tmp);
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    const bool big = pl.L >= (size_t)SPAN;
    launch_weights<P>(ctx, curve, sc, pl, log_n, positions_host, big);
    const uint32_t* tab = sc.at<uint32_t>(pl.o_tab);
    uint32_t *H = sc.at<uint32_t>(pl.o_h), *head = sc.at<uint32_t>(pl.o_head), *tsum = sc.at<uint32_t>(pl.o_tsum);
    const uint32_t ngrp = (pl.k + G - 1) / G;
    hipLaunchKernelGGL(asvc_heads_kernel<P>, dim3(fr_blocks(pl.nseg * ngrp, NT)), dim3(NT), 0, st,
                       reinterpret_cast<const uint32_t*>(phi_dev), tab, pl.k, ngrp, pl.nseg, pl.log_l, H);
    const unsigned cblocks = fr_blocks(pl.nch * pl.k, NT);
    hipLaunchKernelGGL(asvc_scan_chunk_kernel<P>, dim3(cblocks), dim3(NT), 0, st, (const uint32_t*)H, tab, pl.k, pl.nseg, pl.nch, head);
    hipLaunchKernelGGL(asvc_scan_tile_kernel<P>, dim3((unsigned)pl.ntile, pl.k), dim3(NT), 0, st, head, tab, pl.k, pl.nch, tsum);
    hipLaunchKernelGGL(asvc_scan_top_kernel<P>, dim3(pl.k), dim3(NT), 0, st, tsum, tab, pl.k, pl.ntile);
    hipLaunchKernelGGL(asvc_scan_replay_kernel<P>, dim3(cblocks), dim3(NT), 0, st, H, tab, (const uint32_t*)sc.at<uint32_t>(pl.o_c),
                       pl.k, pl.nseg, pl.nch, pl.ntile, (const uint32_t*)head, (const uint32_t*)tsum);
    const unsigned oblocks = fr_blocks((n - k + SPAN - 1) / SPAN, NT);
    uint32_t* q = reinterpret_cast<uint32_t*>(q_dev);
    if (big)
      hipLaunchKernelGGL((asvc_out_kernel<P, true>), dim3(oblocks), dim3(NT), 0, st, (const uint32_t*)H, tab,
                         (const uint32_t*)sc.at<uint32_t>(pl.o_pw), pl.k, n, pl.log_l, q);
    else
      hipLaunchKernelGGL((asvc_out_kernel<P, false>), dim3(oblocks), dim3(NT), 0, st, (const uint32_t*)H, tab, (const uint32_t*)nullptr,
                         pl.k, n, pl.log_l, q);
  });
  ZKP_HIP(hipGetLastError());
}

}  // namespace zkp
