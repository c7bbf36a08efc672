// PLONK prover rounds 2 and 3, the table work (plonk/src/ahp/prover.rs:135-216): the permutation accumulator z of
// PermutationKey::compute_z (ahp/indexer/permutation.rs:67-118) and the third-round quotient of ArithmeticKey::compute_quotient
// (ahp/indexer/arithmetic.rs:53-116), PermutationKey::compute_quotient (permutation.rs:121-169) and prover.rs:184-202.  Fr only,
// so one object serves both curves.
//
// Running product.  out[i] = in[0] ... in[i-1] is blocked: a workgroup owns PLONK_SCAN_BLOCK consecutive elements, a thread
// PLONK_SCAN_ITEMS of them.  One block: the threads' products are scanned in LDS (Hillis-Steele, 8 steps) and every thread
// replays its items from its exclusive prefix.  More blocks: (1) every block leaves its total, (2) the totals are scanned by the
// same code (recursively: a level per factor of PLONK_SCAN_BLOCK), (3) every block replays from its scanned total.  Separate
// launches on one stream: no kernel waits for another workgroup.  Field multiplication is exact and commutative, so the
// blocking does not change a bit of the result.  A thread reads its items in full before it writes them: out may be in.
//
// z.  One pass leaves numerator and denominator of every row in scratch (w^i from one power per thread and one step per row),
// the denominators go through batch_inverse_kernel (poly.hip: Montgomery's trick per lane, a zero stays zero) and the running
// product loads num[i] * (1 / den)[i].  The total of the scan is z[n-1] perm[n-1]: `closes` is total == 1.
//
// Quotient.  One pass over the 4n coset points: thread j owns the points j, j + T, ... (T threads in all, a multiple of 4), so
// x = g w^i is one power per thread and one product by w^T per point, and 1 / (x^n - 1) = 1 / (g^n i^(j mod 4) - 1), i = w^n a
// primitive fourth root, is ONE of four host-computed constants per thread.  18 table reads (z twice) and one write per point.
#include <algorithm>
#include <cstring>

#include "fr_dev.hpp"
#include "internal.hpp"
#include "plonk.hpp"

namespace zkp {

namespace {

constexpr int ST = (int)PLONK_SCAN_THREADS;
constexpr int SI = (int)PLONK_SCAN_ITEMS;
constexpr int QT = (int)PLONK_QUOT_THREADS;

template <class F>
__device__ __forceinline__ F fr_select(bool c, const F& a, const F& b) {
  F r;
#pragma unroll
  for (int i = 0; i < F::N; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// what the running product multiplies: a vector, or num[i] / den[i] with the inverses already taken
template <class F>
struct LoadVec {
  const uint32_t* in;
  __device__ __forceinline__ F operator()(size_t i) const { return F::load(in + i * 8); }
};
template <class F>
struct LoadRatio {
  const uint32_t* num;
  const uint32_t* dinv;
  __device__ __forceinline__ F operator()(size_t i) const { return F::load(num + i * 8) * F::load(dinv + i * 8); }
};

// totals[block] = the product of the block's elements (those below n)
template <class P, class L>
__global__ __launch_bounds__(ST) void scan_totals_kernel(L ld, size_t n, uint32_t* __restrict__ totals) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[ST * 32];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * PLONK_SCAN_BLOCK + (size_t)t * SI;
  F p = base < n ? ld(base) : F::one();
#pragma unroll
  for (int k = 1; k < SI; k++)
    if (base + k < n) p = p * ld(base + k);
  p.store(smem + (size_t)t * 32);
  __syncthreads();
  for (int s = ST / 2; s > 0; s >>= 1) {
    if (t < s) {
      p = p * F::load(smem + (size_t)(t + s) * 32);
      p.store(smem + (size_t)t * 32);
    }
    __syncthreads();
  }
  if (t == 0) p.store(totals + (size_t)blockIdx.x * 8);
}

// out[i] = seed[block] * (the product of the block's elements before i); seeds == NULL: one block, seed 1.
// total_out != NULL: the last thread of the last block leaves the product of everything.
template <class P, class L>
__global__ __launch_bounds__(ST) void scan_apply_kernel(L ld, size_t n, const uint32_t* seeds, uint32_t* out, uint32_t* total_out) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[ST * 32];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * PLONK_SCAN_BLOCK + (size_t)t * SI;
  F x[SI];
#pragma unroll
  for (int k = 0; k < SI; k++) x[k] = base + k < n ? ld(base + k) : F::one();
  F inc = x[0];
#pragma unroll
  for (int k = 1; k < SI; k++) inc = inc * x[k];
  inc.store(smem + (size_t)t * 32);
  __syncthreads();
  for (int d = 1; d < ST; d <<= 1) {                              // inclusive scan of the threads' products
    F o;
    if (t >= d) o = F::load(smem + (size_t)(t - d) * 32);
    __syncthreads();
    if (t >= d) {
      inc = o * inc;
      inc.store(smem + (size_t)t * 32);
    }
    __syncthreads();
  }
  F run = t ? F::load(smem + (size_t)(t - 1) * 32) : F::one();
  if (seeds) run = run * F::load(seeds + (size_t)blockIdx.x * 8);
#pragma unroll
  for (int k = 0; k < SI; k++) {
    if (base + k < n) {
      run.store(out + (base + k) * 8);
      run = run * x[k];
    }
  }
  if (total_out && blockIdx.x == gridDim.x - 1 && t == ST - 1) run.store(total_out);
}

inline size_t scan_blocks(size_t n) { return (n + PLONK_SCAN_BLOCK - 1) / PLONK_SCAN_BLOCK; }

// elements of scratch the levels below n elements need: the totals of every level
size_t scan_scratch_elems(size_t n) {
  size_t e = 0;
  while (n > PLONK_SCAN_BLOCK) {
    n = scan_blocks(n);
    e += n;
  }
  return e;
}

// the exclusive running product of ld(0 .. n) into out, the product of all n into total_dev; launches only
template <class P, class L>
void scan_levels(hipStream_t st, L ld, size_t n, uint32_t* out, uint32_t* scratch, uint32_t* total_dev) {
  using F = Fp<P>;
  if (n <= PLONK_SCAN_BLOCK) {
    hipLaunchKernelGGL((scan_apply_kernel<P, L>), dim3(1), dim3(ST), 0, st, ld, n, (const uint32_t*)nullptr, out, total_dev);
    return;
  }
  const size_t nblk = scan_blocks(n);
  uint32_t* totals = scratch;
  hipLaunchKernelGGL((scan_totals_kernel<P, L>), dim3((unsigned)nblk), dim3(ST), 0, st, ld, n, totals);
  scan_levels<P, LoadVec<F>>(st, LoadVec<F>{totals}, nblk, totals, scratch + nblk * 8, total_dev);
  hipLaunchKernelGGL((scan_apply_kernel<P, L>), dim3((unsigned)nblk), dim3(ST), 0, st, ld, n, (const uint32_t*)totals, out,
                     (uint32_t*)nullptr);
}

struct PermPtrs {
  const uint32_t* w[4];
  const uint32_t* s[4];
};
enum { PZ_KB = 0, PZ_BETA = 4, PZ_GAMMA, PZ_W, PZ_WT, PZ_COUNT };

// num[i] = prod_s (w_s[i] + ks_s beta w^i + gamma), den[i] = prod_s (w_s[i] + beta sigma_s[i] + gamma); thread j: rows j, j + T, ...
template <class P>
__global__ __launch_bounds__(QT) void perm_terms_kernel(PermPtrs p, size_t n, size_t T, FrArgs<Fp<P>, PZ_COUNT> c,
                                                        uint32_t* __restrict__ num, uint32_t* __restrict__ den) {
  using F = Fp<P>;
  const size_t j = (size_t)blockIdx.x * QT + threadIdx.x;
  if (j >= T) return;
  const F beta = c.get(PZ_BETA), gamma = c.get(PZ_GAMMA), wT = c.get(PZ_WT);
  F x = c.get(PZ_W).pow_u64(j);
  for (size_t i = j; i < n; i += T) {
    F nu, de;
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const F wg = F::load(p.w[s] + i * 8) + gamma;
      const F a = wg + c.get(PZ_KB + s) * x;
      const F b = wg + beta * F::load(p.s[s] + i * 8);
      nu = s ? nu * a : a;
      de = s ? de * b : b;
    }
    nu.store(num + i * 8);
    de.store(den + i * 8);
    x = x * wT;
  }
}

struct QuotPtrs {
  const uint32_t* w[4];
  const uint32_t* z;
  const uint32_t* pi;
  const uint32_t* q[7];                                          // q_0, q_1, q_2, q_3, q_m, q_c, q_arith
  const uint32_t* s[4];
  const uint32_t* l1;
};
enum { QC_KB = 0, QC_BETA = 4, QC_GAMMA, QC_ALPHA, QC_ALPHA2, QC_VINV, QC_G = QC_VINV + 4, QC_W, QC_WT, QC_COUNT };

// t[i] = (t_arith[i] + t_perm[i]) / (x_i^n - 1), x_i = g w^i over the N = 4n coset points; thread j: points j, j + T, ...
template <class P>
__global__ __launch_bounds__(QT) void quotient_kernel(QuotPtrs p, size_t N, size_t T, FrArgs<Fp<P>, QC_COUNT> c,
                                                      uint32_t* __restrict__ out) {
  using F = Fp<P>;
  const size_t j = (size_t)blockIdx.x * QT + threadIdx.x;
  if (j >= T) return;
  const F beta = c.get(QC_BETA), gamma = c.get(QC_GAMMA), wT = c.get(QC_WT);
  // T is a multiple of 4: i mod 4 == j mod 4 for every point of this thread
  const F vinv = fr_select((j & 2) != 0, fr_select((j & 1) != 0, c.get(QC_VINV + 3), c.get(QC_VINV + 2)),
                           fr_select((j & 1) != 0, c.get(QC_VINV + 1), c.get(QC_VINV + 0)));
  F x = c.get(QC_G) * c.get(QC_W).pow_u64(j);
  for (size_t i = j; i < N; i += T) {
    F w[4];
#pragma unroll
    for (int s = 0; s < 4; s++) w[s] = F::load(p.w[s] + i * 8);
    // (q_0 w_0 + q_1 w_1 + q_2 w_2 + q_3 w_3 + q_m w_1 w_2 + q_c + pi) q_arith: zero where q_arith is
    F acc = F::load(p.q[4] + i * 8) * w[1] * w[2] + F::load(p.q[5] + i * 8) + F::load(p.pi + i * 8);
#pragma unroll
    for (int s = 0; s < 4; s++) acc = acc + F::load(p.q[s] + i * 8) * w[s];
    acc = acc * F::load(p.q[6] + i * 8);
    const F z = F::load(p.z + i * 8);
    acc = acc + (z - F::one()) * F::load(p.l1 + i * 8) * c.get(QC_ALPHA2);
    F nu = z, de = F::load(p.z + ((i + 4) & (N - 1)) * 8);        // the accumulator one row on: 4 coset points, wrapping
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const F wg = w[s] + gamma;
      nu = nu * (wg + c.get(QC_KB + s) * x);
      de = de * (wg + beta * F::load(p.s[s] + i * 8));
    }
    acc = acc + (nu - de) * c.get(QC_ALPHA);
    (acc * vinv).store(out + i * 8);
    x = x * wT;
  }
}

int fr_two_adicity(int curve) { return curve == ZKP_BN254 ? hostf::consts::Bn254Fr::TWO_ADICITY : hostf::consts::Bls381Fr::TWO_ADICITY; }

// the generator of the domain of size 2^log that zkp_ntt_dev uses (ntt.hip ntt_setup_kernel), and the coset generator
hostf::FrE host_root(const hostf::HostField& fr, int curve, int log) {
  hostf::FrE e{};
  memcpy(e.data(), curve == ZKP_BN254 ? hostf::consts::Bn254Fr::ROOT : hostf::consts::Bls381Fr::ROOT, 32);
  return fr.pow2k(e, fr_two_adicity(curve) - log);
}
hostf::FrE host_coset_gen(int curve) {
  hostf::FrE e{};
  memcpy(e.data(), curve == ZKP_BN254 ? hostf::consts::Bn254Fr::GEN : hostf::consts::Bls381Fr::GEN, 32);
  return e;
}

// the rules every PLONK call shares: n = 2^log_n rows with log_n >= 2, and a domain of 4n points
void require_plonk_domain(int curve, uint32_t log_n) {
  ZKP_REQUIRE(log_n >= 2, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(log_n + 2 <= (uint32_t)fr_two_adicity(curve), ZKP_ERR_DOMAIN_TOO_LARGE);
}

// threads of the two row kernels: every row its own thread up to the cap; a power of two, a multiple of 4 for n >= 4
size_t row_threads(size_t n) { return std::min(n, (size_t)PLONK_QUOT_THREADS * PLONK_QUOT_MAX_BLOCKS); }

}  // namespace

void fr_prefix_product(zkp_ctx* ctx, int curve, const uint64_t* in_dev, uint64_t* out_dev, size_t n, uint64_t* total_out_host) {
  fr_require_curve(curve);
  ZKP_REQUIRE(in_dev && out_dev, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(n >= 1 && n <= ((size_t)1 << PLONK_SCAN_MAX_LOG), ZKP_ERR_BAD_ARG);
  require_aligned16(in_dev);
  require_aligned16(out_dev);
  ZKP_REQUIRE(same_or_disjoint((uintptr_t)in_dev, n * 32, (uintptr_t)out_dev, n * 32), ZKP_ERR_BAD_ARG);
  hipStream_t st = ctx->cur->stream;
  Scratch sc;
  const size_t o_tot = sc.take(32), o_lv = sc.take(scan_scratch_elems(n) * 32);
  sc.resolve(ctx->poly_tmp);
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    scan_levels<P, LoadVec<Fp<P>>>(st, LoadVec<Fp<P>>{reinterpret_cast<const uint32_t*>(in_dev)}, n, reinterpret_cast<uint32_t*>(out_dev),
                                   sc.at<uint32_t>(o_lv), sc.at<uint32_t>(o_tot));
  });
  ZKP_HIP(hipGetLastError());
  if (total_out_host) ZKP_HIP(hipMemcpyAsync(total_out_host, sc.at<uint32_t>(o_tot), 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

void fr_plonk_perm_z(zkp_ctx* ctx, int curve, const uint64_t* const* w_dev, const uint64_t* const* sigma_dev, uint32_t log_n,
                     const uint64_t* ks_host, const uint64_t* beta_host, const uint64_t* gamma_host, uint64_t* z_out_dev,
                     int32_t* closes_out_host) {
  fr_require_curve(curve);
  ZKP_REQUIRE(w_dev && sigma_dev && ks_host && beta_host && gamma_host && z_out_dev && closes_out_host, ZKP_ERR_BAD_ARG);
  PermPtrs pp{};
  for (int s = 0; s < 4; s++) {
    ZKP_REQUIRE(w_dev[s] && sigma_dev[s], ZKP_ERR_BAD_ARG);
    require_aligned16(w_dev[s]);
    require_aligned16(sigma_dev[s]);
    pp.w[s] = reinterpret_cast<const uint32_t*>(w_dev[s]);
    pp.s[s] = reinterpret_cast<const uint32_t*>(sigma_dev[s]);
  }
  require_aligned16(z_out_dev);
  require_plonk_domain(curve, log_n);
  fr_require_canonical(curve, ks_host, 4);
  fr_require_canonical(curve, beta_host, 1);
  fr_require_canonical(curve, gamma_host, 1);
  const size_t n = (size_t)1 << log_n, T = row_threads(n);
  const hostf::HostField fr = hostf::fr_field(curve);
  const hostf::FrE beta = fr_host_load(beta_host), w = host_root(fr, curve, (int)log_n);
  hipStream_t st = ctx->cur->stream;
  Scratch sc;                                                    // z_out is written last, from scratch only: it may be an input
  const size_t o_tot = sc.take(32), o_num = sc.take(n * 32), o_den = sc.take(n * 32), o_lv = sc.take(scan_scratch_elems(n) * 32);
  sc.resolve(ctx->poly_tmp);
  uint32_t* num = sc.at<uint32_t>(o_num);
  uint32_t* den = sc.at<uint32_t>(o_den);
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    using F = Fp<P>;
    FrArgs<F, PZ_COUNT> c;
    for (int s = 0; s < 4; s++) c.set(PZ_KB + s, fr.mul(fr_host_load(ks_host + 4 * s), beta));
    c.set(PZ_BETA, beta);
    c.set(PZ_GAMMA, fr_host_load(gamma_host));
    c.set(PZ_W, w);
    c.set(PZ_WT, fr.pow2k(w, log2_ceil(T)));
    hipLaunchKernelGGL(perm_terms_kernel<P>, dim3(fr_blocks(T, QT)), dim3(QT), 0, st, pp, n, T, c, num, den);
  });
  ZKP_HIP(hipGetLastError());
  fr_batch_inverse(ctx, curve, reinterpret_cast<uint64_t*>(den), n);
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    scan_levels<P, LoadRatio<Fp<P>>>(st, LoadRatio<Fp<P>>{num, den}, n, reinterpret_cast<uint32_t*>(z_out_dev), sc.at<uint32_t>(o_lv),
                                     sc.at<uint32_t>(o_tot));
  });
  ZKP_HIP(hipGetLastError());
  hostf::FrE total{};
  ZKP_HIP(hipMemcpyAsync(total.data(), sc.at<uint32_t>(o_tot), 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
  *closes_out_host = total == fr.one_() ? 1 : 0;                // the assert_eq! of permutation.rs:112
}

void fr_plonk_quotient(zkp_ctx* ctx, int curve, const uint64_t* const* w_4n, const uint64_t* z_4n, const uint64_t* pi_4n,
                       const uint64_t* const* q_4n, const uint64_t* const* sigma_4n, const uint64_t* l1_4n, uint32_t log_n,
                       const uint64_t* ks_host, const uint64_t* beta_host, const uint64_t* gamma_host, const uint64_t* alpha_host,
                       uint64_t* t_out_dev) {
  fr_require_curve(curve);
  ZKP_REQUIRE(w_4n && z_4n && pi_4n && q_4n && sigma_4n && l1_4n && t_out_dev, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(ks_host && beta_host && gamma_host && alpha_host, ZKP_ERR_BAD_ARG);
  require_plonk_domain(curve, log_n);
  const size_t n = (size_t)1 << log_n, N = 4 * n, T = row_threads(N);
  QuotPtrs qp{};
  const uint64_t* in[18];
  for (int s = 0; s < 4; s++) {
    in[s] = w_4n[s];
    in[4 + s] = sigma_4n[s];
  }
  for (int s = 0; s < 7; s++) in[8 + s] = q_4n[s];
  in[15] = z_4n;
  in[16] = pi_4n;
  in[17] = l1_4n;
  require_aligned16(t_out_dev);
  std::vector<MemSpan> spans = {fr_span(t_out_dev, N, true)};    // point i + 4 of z is read after point i is written
  for (int k = 0; k < 18; k++) {
    ZKP_REQUIRE(in[k] != nullptr, ZKP_ERR_BAD_ARG);
    require_aligned16(in[k]);
    spans.push_back(fr_span(in[k], N, false));
  }
  require_disjoint_outputs(std::move(spans));
  for (int s = 0; s < 4; s++) {
    qp.w[s] = reinterpret_cast<const uint32_t*>(w_4n[s]);
    qp.s[s] = reinterpret_cast<const uint32_t*>(sigma_4n[s]);
  }
  for (int s = 0; s < 7; s++) qp.q[s] = reinterpret_cast<const uint32_t*>(q_4n[s]);
  qp.z = reinterpret_cast<const uint32_t*>(z_4n);
  qp.pi = reinterpret_cast<const uint32_t*>(pi_4n);
  qp.l1 = reinterpret_cast<const uint32_t*>(l1_4n);
  fr_require_canonical(curve, ks_host, 4);
  fr_require_canonical(curve, beta_host, 1);
  fr_require_canonical(curve, gamma_host, 1);
  fr_require_canonical(curve, alpha_host, 1);
  const hostf::HostField fr = hostf::fr_field(curve);
  const hostf::FrE beta = fr_host_load(beta_host), alpha = fr_host_load(alpha_host);
  const hostf::FrE w = host_root(fr, curve, (int)log_n + 2), g = host_coset_gen(curve);
  // v_4n_inversed (ahp/indexer/mod.rs:223-225): x_i^n - 1 = g^n (w^n)^i - 1 takes four values
  const hostf::FrE iota = fr.pow2k(w, (int)log_n);
  hostf::FrE gn = fr.pow2k(g, (int)log_n);
  hipStream_t st = ctx->cur->stream;
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    using F = Fp<P>;
    FrArgs<F, QC_COUNT> c;
    for (int s = 0; s < 4; s++) c.set(QC_KB + s, fr.mul(fr_host_load(ks_host + 4 * s), beta));
    c.set(QC_BETA, beta);
    c.set(QC_GAMMA, fr_host_load(gamma_host));
    c.set(QC_ALPHA, alpha);
    c.set(QC_ALPHA2, fr.mul(alpha, alpha));
    for (int k = 0; k < 4; k++) {
      c.set(QC_VINV + k, fr.inverse(fr.sub(gn, fr.one_())));
      gn = fr.mul(gn, iota);
    }
    c.set(QC_G, g);
    c.set(QC_W, w);
    c.set(QC_WT, fr.pow2k(w, log2_ceil(T)));
    hipLaunchKernelGGL(quotient_kernel<P>, dim3(fr_blocks(T, QT)), dim3(QT), 0, st, qp, N, T, c,
                       reinterpret_cast<uint32_t*>(t_out_dev));
  });
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipStreamSynchronize(st));
}

}  // namespace zkp
