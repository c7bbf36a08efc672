// What a PLONK prover does with its coefficient vectors after round 3 (plonk/src/lib.rs:93-204): it evaluates them at the
// verifier's points (EvaluationsProvider::get_lc_eval, ahp/evaluations.rs:24-49) and opens linear combinations of them
// (the polynomial of an ark_poly_commit LinearCombination, then a division by X - z in poly.hip).  Fr only, so one object
// serves both curves.
//
// Evaluation of `count` polynomials at ONE point z.  One pass reads every coefficient once: thread j of T owns the indices
// j, j + T, ..., so a wavefront's 16-byte loads are consecutive.  The thread forms z^j with one pow_u64 and steps by z^T (computed
// once on the host); each power multiplies the coefficient of every polynomial that is still in range.  The accumulators of
// FR_OPEN_EVAL_GROUP polynomials stay in registers; the next group restarts the power chain from the kept z^j.  Every workgroup
// leaves one partial per polynomial through fr_block_sum; a second launch adds a polynomial's partials with one workgroup per
// polynomial.  Separate launches on one stream: no kernel waits for another workgroup.  Field addition is exact and every
// element written is canonical, so the blocking does not change a bit of the result.  z^0 = 1 also for z = 0 (pow_u64(0) is 1).
//
// Linear combination.  out[i] = sum_{k : i < ns[k]} c_k p_k[i] in one element-wise launch.  The scalars and the pointer / length
// table are kernel arguments: uniform operands, no staging copy.  A thread reads index i of every input before it writes out[i]
// and touches no other index, so out may be one of the inputs (same base).
#include <algorithm>
#include <cstring>

#include "fr_dev.hpp"
#include "fr_open.hpp"
#include "internal.hpp"

namespace zkp {

namespace {

constexpr int ET = (int)FR_OPEN_EVAL_THREADS;
constexpr int EG = (int)FR_OPEN_EVAL_GROUP;
constexpr int LT = (int)FR_OPEN_LINCOMB_THREADS;
constexpr int MAXP = (int)FR_OPEN_MAX_POLYS;

// the vectors of a call: unused entries are NULL with length 0
struct OpenTable {
  const uint32_t* p[MAXP];
  uint32_t n[MAXP];
};

// partial[k * gridDim.x + block] = sum over the block's threads j of sum_{i = j, j + T, ... < n[k]} p_k[i] z^i,  T = gridDim.x * ET
template <class P>
__global__ __launch_bounds__(ET) void eval_many_kernel(OpenTable tb, uint32_t count, FrArgs<Fp<P>, 2> c, uint32_t* __restrict__ partial) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[EG * ET * 32];
  const size_t T = (size_t)gridDim.x * ET;
  const size_t j = (size_t)blockIdx.x * ET + threadIdx.x;
  const F zT = c.get(1);
  const F zj = c.get(0).pow_u64(j);
  for (uint32_t g = 0; g < count; g += EG) {
    uint32_t len[EG];
    const uint32_t* p[EG];
    uint32_t nmax = 0;
#pragma unroll
    for (int k = 0; k < EG; k++) {                               // g + k < MAXP: MAXP is a multiple of EG
      len[k] = tb.n[g + k];
      p[k] = tb.p[g + k];
      nmax = len[k] > nmax ? len[k] : nmax;
    }
    F acc[EG];
#pragma unroll
    for (int k = 0; k < EG; k++) acc[k] = F::zero();
    F x = zj;
    for (size_t i = j; i < nmax; i += T) {
#pragma unroll
      for (int k = 0; k < EG; k++)
        if (i < len[k]) acc[k] = acc[k] + F::load(p[k] + i * 8) * x;
      x = x * zT;
    }
    fr_block_sum<F, ET, EG>(acc, smem);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < EG; k++)
        if (g + k < count) acc[k].store(partial + ((size_t)(g + k) * gridDim.x + blockIdx.x) * 8);
    }
  }
}

// out[i] = sum_{k < count, i < n[k]} c_k p_k[i]; every term has n[k] >= 1 and c_k != 0 (the host dropped the others)
template <class P>
__global__ __launch_bounds__(LT) void lincomb_kernel(OpenTable tb, uint32_t count, FrArgs<Fp<P>, MAXP> c, uint32_t* out, size_t n_out) {
  using F = Fp<P>;
  const size_t i = (size_t)blockIdx.x * LT + threadIdx.x;
  if (i >= n_out) return;
  F acc = F::zero();
  for (uint32_t k = 0; k < count; k++)
    if (i < tb.n[k]) acc = acc + c.get(k) * F::load(tb.p[k] + i * 8);
  acc.store(out + i * 8);
}

// the rules both entries share; returns the longest length
size_t require_table(size_t count, const uint64_t* const* p_dev, const size_t* ns) {
  ZKP_REQUIRE(count >= 1 && count <= FR_OPEN_MAX_POLYS, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(p_dev && ns, ZKP_ERR_BAD_ARG);
  size_t nmax = 0;
  for (size_t k = 0; k < count; k++) {
    ZKP_REQUIRE(ns[k] <= ((size_t)1 << FR_OPEN_MAX_LOG), ZKP_ERR_BAD_ARG);
    if (ns[k] == 0) continue;                                    // the zero polynomial: its pointer is never read
    ZKP_REQUIRE(p_dev[k] != nullptr, ZKP_ERR_BAD_ARG);
    require_aligned16(p_dev[k]);
    nmax = std::max(nmax, ns[k]);
  }
  return nmax;
}

}  // namespace

void fr_poly_eval_many(zkp_ctx* ctx, int curve, size_t count, const uint64_t* const* p_dev, const size_t* ns, const uint64_t* z_host,
                       uint64_t* out_host) {
  fr_require_curve(curve);
  ZKP_REQUIRE(z_host && out_host, ZKP_ERR_BAD_ARG);
  const size_t nmax = require_table(count, p_dev, ns);
  fr_require_canonical(curve, z_host, 1);
  OpenTable tb{};
  for (size_t k = 0; k < count; k++) {
    tb.n[k] = (uint32_t)ns[k];
    tb.p[k] = ns[k] ? reinterpret_cast<const uint32_t*>(p_dev[k]) : nullptr;
  }
  const uint32_t nwg = (uint32_t)std::min<size_t>(std::max<size_t>((nmax + ET - 1) / ET, 1), FR_OPEN_EVAL_MAX_BLOCKS);
  const hostf::HostField fr = hostf::fr_field(curve);
  const hostf::FrE z = fr_host_load(z_host), zT = fr.pow(z, (uint64_t)nwg * ET);
  hipStream_t st = ctx->cur->stream;
  Scratch sc;
  const size_t o_out = sc.take(count * 32), o_part = sc.take(count * (size_t)nwg * 32);
  sc.resolve(ctx->poly_tmp);
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    FrArgs<Fp<P>, 2> c;
    c.set(0, z);
    c.set(1, zT);
    hipLaunchKernelGGL(eval_many_kernel<P>, dim3(nwg), dim3(ET), 0, st, tb, (uint32_t)count, c, sc.at<uint32_t>(o_part));
    fr_sum_partials<P, ET>(st, sc.at<uint32_t>(o_part), nwg, (uint32_t)count, sc.at<uint32_t>(o_out));
  });
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipMemcpyAsync(out_host, sc.at<uint32_t>(o_out), count * 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

void fr_lincomb(zkp_ctx* ctx, int curve, size_t count, const uint64_t* const* p_dev, const size_t* ns, const uint64_t* coeffs_host,
                uint64_t* out_dev, size_t n_out) {
  fr_require_curve(curve);
  ZKP_REQUIRE(coeffs_host && out_dev, ZKP_ERR_BAD_ARG);
  const size_t nmax = require_table(count, p_dev, ns);
  ZKP_REQUIRE(n_out >= 1 && n_out <= ((size_t)1 << FR_OPEN_MAX_LOG) && nmax <= n_out, ZKP_ERR_BAD_ARG);
  require_aligned16(out_dev);
  for (size_t k = 0; k < count; k++) {
    if (ns[k] == 0) continue;
    ZKP_REQUIRE(same_or_disjoint((uintptr_t)p_dev[k], ns[k] * 32, (uintptr_t)out_dev, n_out * 32), ZKP_ERR_BAD_ARG);
  }
  fr_require_canonical(curve, coeffs_host, count);
  hipStream_t st = ctx->cur->stream;
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    OpenTable tb{};
    FrArgs<Fp<P>, MAXP> c{};
    uint32_t used = 0;
    for (size_t k = 0; k < count; k++) {
      const uint64_t* ck = coeffs_host + 4 * k;
      if (ns[k] == 0 || !(ck[0] | ck[1] | ck[2] | ck[3])) continue;       // a zero term: dropped here
      tb.p[used] = reinterpret_cast<const uint32_t*>(p_dev[k]);
      tb.n[used] = (uint32_t)ns[k];
      c.set((int)used++, ck);
    }
    if (!used) {
      ZKP_HIP(hipMemsetAsync(out_dev, 0, n_out * 32, st));
      return;
    }
    hipLaunchKernelGGL(lincomb_kernel<P>, dim3((unsigned)((n_out + LT - 1) / LT)), dim3(LT), 0, st, tb, used, c,
                       reinterpret_cast<uint32_t*>(out_dev), n_out);
  });
  ZKP_HIP(hipGetLastError());
}

}  // namespace zkp
