// SPARK memory checking on the device (zkp_fr_memcheck_circuits_dev / zkp_fr_product_circuit_dev): circuit_hash and
// construct_product_circuit of memory_checking (spartan/src/spark.rs:209-347), every layer kept for product_circuit_eval_prover
// (prover.rs:1313-1440).  Fr only, so one object serves both curves (Bn254Fr / Bls381Fr).
//
// A circuit of n leaves is ONE buffer of 2n - 2 elements: layer l (n >> l elements) starts at element 2n - (2n >> l); the
// reference's left_vec[l] / right_vec[l] are its first / second half, so layer[l+1][j] = layer[l][j] * layer[l][j + len/2] and
// layer[l+k][j] is the product of the 2^k elements layer[l][j + s (len >> k)].
//
// Strided pass (radix 2^RL, RL = 3 unless fewer layers remain above the tail): with s = len >> RL, thread j < s of circuit
// blockIdx.y loads the 2^RL elements j + i s (32 contiguous bytes per thread, contiguous across j), forms 4 + 2 + 1 products in
// place in its registers and stores each into the layer it belongs to: three layers per launch, 32 B read and 28 B written per
// input element instead of 56 B and 28 B over three launches.  Every position of the four layers belongs to exactly one thread.
//
// Leaf pass (HASH): the first launch of zkp_fr_memcheck_circuits_dev computes its inputs instead of loading them,
//   leaf = addr gamma1^2 + val gamma1 + ts + ts_add - gamma2,
// and stores them as layer 0.  addr and ts are raw 32-bit integers: the Montgomery product of the integer a with the constant
// gamma1^2 R^2 is a gamma1^2 R, and ts R2 likewise, so no separate to-Montgomery product is spent.  Entries that share (addr, val,
// ts) and differ in ts_add (the read and write circuits of a list) form one group: hashed once, + 1 for the second circuit.
//
// Tail: a layer of <= 2^SP_TAIL_LOG elements is finished by ONE workgroup per circuit (per group with HASH): a thread keeps its
// product, publishes it in LDS, and after one __syncthreads() per layer multiplies it with its partner's; every layer goes to global
// memory, the root to a device slot.  One D2H copy of `count` roots ends the call.  No workgroup waits on another.
#include <algorithm>
#include <cstring>
#include <vector>

#include "fr_dev.hpp"
#include "spark.hpp"

namespace zkp {

namespace {

constexpr int SP_THREADS = 256;
static_assert((1 << SP_TAIL_LOG) <= 2 * SP_THREADS, "the tail takes one product per thread in its first layer");

struct SpGroup {             // circuits that share their inputs: out[a] has ts_add == a (or is NULL), root slot idx[a]
  const uint32_t* addr;      // NULL: the leaf's own index
  const uint32_t* val;
  const uint32_t* ts;        // NULL: 0
  uint32_t* out[2];
  uint32_t idx[2];
};

template <class F>
struct SpConsts {
  FrArg<F> g1sq_r, g1, g2;   // gamma1^2 R (as a Montgomery word: gamma1^2 R^2), gamma1, gamma2
};

template <class F>
__device__ __forceinline__ F sp_raw(uint32_t a) {          // the integer a as limbs: NOT Montgomery
  F x = F::zero();
  x.v[0] = a;
  return x;
}

// circuit_hash(addr, val, ts)[i] - gamma2 (spark.rs:298-312, 250-273), ts_add not yet added
template <class F>
__device__ __forceinline__ F sp_leaf(const SpGroup& g, size_t i, const F& g1sq_r, const F& g1, const F& g2) {
  F h = F::load(g.val + i * 8) * g1 + sp_raw<F>(g.addr ? g.addr[i] : (uint32_t)i) * g1sq_r;
  if (g.ts) h = h + sp_raw<F>(g.ts[i]) * F::r2();
  return h - g2;
}

// e: the 2^RL elements j + i s of layer l; stores the products into layers l + 1 .. l + RL of buf
template <class F, int RL>
__device__ __forceinline__ void sp_products(F (&e)[1 << RL], uint32_t* buf, size_t n, uint32_t l, size_t j, size_t s) {
#pragma unroll
  for (int lv = 1; lv <= RL; lv++) {
    uint32_t* dst = buf + sp_layer_offset(n, (int)l + lv) * 8;
#pragma unroll
    for (int i = 0; i < (1 << (RL - lv)); i++) {
      e[i] = e[i] * e[i + (1 << (RL - lv))];
      e[i].store(dst + (j + (size_t)i * s) * 8);
    }
  }
}

// grid (ceil(s / SP_THREADS), groups or circuits), s = (n >> l) >> RL >= 1.  HASH: l == 0, blockIdx.y is a group.
template <class P, int RL, bool HASH>
__global__ __launch_bounds__(SP_THREADS) void sp_pass_kernel(const SpGroup* __restrict__ groups, uint32_t* const* __restrict__ circ,
                                                             size_t n, uint32_t l, SpConsts<Fp<P>> k) {
  using F = Fp<P>;
  constexpr int R = 1 << RL;
  const size_t s = (n >> l) >> RL;
  const size_t j = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (j >= s) return;
  if (HASH) {
    const SpGroup g = groups[blockIdx.y];
    const F g1sq_r = k.g1sq_r.get(), g1 = k.g1.get(), g2 = k.g2.get();
    F base[R];
#pragma unroll
    for (int i = 0; i < R; i++) base[i] = sp_leaf<F>(g, j + (size_t)i * s, g1sq_r, g1, g2);
    for (int a = 0; a < 2; a++) {
      uint32_t* buf = a ? g.out[1] : g.out[0];      // selects, not a dynamic index: g stays in registers
      if (!buf) continue;
      F e[R];
#pragma unroll
      for (int i = 0; i < R; i++) {
        e[i] = a ? base[i] + F::one() : base[i];
        e[i].store(buf + (j + (size_t)i * s) * 8);
      }
      sp_products<F, RL>(e, buf, n, 0, j, s);
    }
  } else {
    uint32_t* buf = circ[blockIdx.y];
    const uint32_t* src = buf + sp_layer_offset(n, (int)l) * 8;
    F e[R];
#pragma unroll
    for (int i = 0; i < R; i++) e[i] = F::load(src + (j + (size_t)i * s) * 8);
    sp_products<F, RL>(e, buf, n, l, j, s);
  }
}

// one workgroup per circuit (HASH: per group, l == 0): layers l + 1 .. of a layer l of len = n >> l <= 2^SP_TAIL_LOG elements, and the root
template <class P, bool HASH>
__global__ __launch_bounds__(SP_THREADS) void sp_tail_kernel(const SpGroup* __restrict__ groups, uint32_t* const* __restrict__ circ,
                                                             size_t n, uint32_t l, SpConsts<Fp<P>> k, uint32_t* __restrict__ roots) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[SP_THREADS * 32];
  const uint32_t t = threadIdx.x;
  const uint32_t half = (uint32_t)((n >> l) >> 1);          // 1 .. SP_THREADS
  SpGroup g;
  F a0 = F::zero(), b0 = F::zero();
  if (HASH) {
    g = groups[blockIdx.x];
    if (t < half) {
      const F g1sq_r = k.g1sq_r.get(), g1 = k.g1.get(), g2 = k.g2.get();
      a0 = sp_leaf<F>(g, t, g1sq_r, g1, g2);
      b0 = sp_leaf<F>(g, t + half, g1sq_r, g1, g2);
    }
  } else {
    g.out[0] = circ[blockIdx.x];
    g.out[1] = nullptr;
    g.idx[0] = blockIdx.x;
    if (t < half) {
      const uint32_t* src = g.out[0] + sp_layer_offset(n, (int)l) * 8;
      a0 = F::load(src + (size_t)t * 8);
      b0 = F::load(src + (size_t)(t + half) * 8);
    }
  }
  for (int a = 0; a < (HASH ? 2 : 1); a++) {
    uint32_t* buf = a ? g.out[1] : g.out[0];      // selects, not a dynamic index: g stays in registers
    if (!buf) continue;                                      // uniform over the workgroup
    F p = F::zero();
    if (t < half) {
      F x = a0, y = b0;
      if (HASH) {
        if (a) {
          x = x + F::one();
          y = y + F::one();
        }
        x.store(buf + (size_t)t * 8);
        y.store(buf + (size_t)(t + half) * 8);
      }
      p = x * y;
    }
    // p of thread t < cur is element t of layer lv (cur elements); cur == 1: the root
    uint32_t lv = l + 1;
    for (uint32_t cur = half; cur > 1; cur >>= 1, lv++) {
      if (t < cur) {
        p.store(buf + (sp_layer_offset(n, (int)lv) + t) * 8);
        p.store(smem + (size_t)t * 32);
      }
      __syncthreads();
      // reads [cur / 2, cur); the next layer writes [0, cur / 2): one barrier per layer is enough
      if (t < cur / 2) p = p * F::load(smem + (size_t)(t + cur / 2) * 32);
    }
    if (t == 0) p.store(roots + (size_t)(a ? g.idx[1] : g.idx[0]) * 8);
    __syncthreads();                                         // the second circuit of the group reuses smem
  }
}

template <class P, bool HASH>
void launch_pass(hipStream_t st, int rl, dim3 grid, const SpGroup* groups, uint32_t* const* circ, size_t n, uint32_t l,
                 const SpConsts<Fp<P>>& k) {
  const dim3 block(SP_THREADS);
  if (rl == 3) hipLaunchKernelGGL((sp_pass_kernel<P, 3, HASH>), grid, block, 0, st, groups, circ, n, l, k);
  else if (rl == 2) hipLaunchKernelGGL((sp_pass_kernel<P, 2, HASH>), grid, block, 0, st, groups, circ, n, l, k);
  else hipLaunchKernelGGL((sp_pass_kernel<P, 1, HASH>), grid, block, 0, st, groups, circ, n, l, k);
}

template <class P>
void circuits_t(zkp_ctx* ctx, const std::vector<SpGroup>& groups, size_t count, uint64_t* const* circuits, size_t n,
                const SpConsts<Fp<P>>& k, uint64_t* roots_host) {
  const bool hash = !groups.empty();
  hipStream_t st = ctx->cur->stream;
  Scratch sc;
  const size_t o_groups = sc.take(groups.size() * sizeof(SpGroup)), o_circ = sc.take(count * sizeof(uint32_t*));
  const size_t o_roots = sc.take(count * 32);
  sc.resolve(ctx->poly_tmp);
  SpGroup* d_groups = sc.at<SpGroup>(o_groups);
  uint32_t** d_circ = sc.at<uint32_t*>(o_circ);
  uint32_t* d_roots = sc.at<uint32_t>(o_roots);
  if (hash) ZKP_HIP(hipMemcpyAsync(d_groups, groups.data(), groups.size() * sizeof(SpGroup), hipMemcpyHostToDevice, st));
  ZKP_HIP(hipMemcpyAsync(d_circ, circuits, count * sizeof(uint32_t*), hipMemcpyHostToDevice, st));

  const int log_n = log2_ceil(n);
  // strided passes down to 2^SP_TAIL_LOG elements: radix 8 first (the longest layers), the remainder (radix 2 or 4) last
  uint32_t l = 0;
  for (int rem = log_n - SP_TAIL_LOG; rem > 0;) {
    const int rl = std::min(rem, 3);
    const size_t s = (n >> l) >> rl;
    const bool h = hash && l == 0;
    const dim3 grid(fr_blocks(s, SP_THREADS), (unsigned)(h ? groups.size() : count));
    if (h) launch_pass<P, true>(st, rl, grid, d_groups, d_circ, n, l, k);
    else launch_pass<P, false>(st, rl, grid, d_groups, d_circ, n, l, k);
    l += rl;
    rem -= rl;
  }
  if (hash && l == 0)
    hipLaunchKernelGGL((sp_tail_kernel<P, true>), dim3((unsigned)groups.size()), dim3(SP_THREADS), 0, st, d_groups, d_circ, n, l, k, d_roots);
  else
    hipLaunchKernelGGL((sp_tail_kernel<P, false>), dim3((unsigned)count), dim3(SP_THREADS), 0, st, d_groups, d_circ, n, l, k, d_roots);
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipMemcpyAsync(roots_host, d_roots, count * 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

}  // namespace

void fr_spark_circuits(zkp_ctx* ctx, int curve, size_t count, const uint32_t* const* addr_dev, const uint64_t* const* val_dev,
                       const uint32_t* const* ts_dev, const uint32_t* ts_add, uint64_t* const* circuits_dev, size_t n,
                       const uint64_t* gamma1_host, const uint64_t* gamma2_host, uint64_t* roots_host) {
  const bool hash = val_dev != nullptr;
  fr_require_curve(curve);
  ZKP_REQUIRE(count >= 1 && count <= SP_MAX_CIRCUITS, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(is_pow2(n) && n >= 2 && n <= ((size_t)1 << SP_MAX_LOG), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(circuits_dev && roots_host, ZKP_ERR_BAD_ARG);
  const hostf::HostField fr = hostf::fr_field(curve);
  hostf::FrE g1{}, g2{};
  if (hash) {
    ZKP_REQUIRE(addr_dev && ts_dev && ts_add && gamma1_host && gamma2_host, ZKP_ERR_BAD_ARG);
    fr_require_canonical(curve, gamma1_host, 1);
    fr_require_canonical(curve, gamma2_host, 1);
    g1 = fr_host_load(gamma1_host);
    g2 = fr_host_load(gamma2_host);
  }
  // circuit buffers overlap nothing; inputs may overlap each other (shared between entries)
  std::vector<MemSpan> spans;
  spans.reserve(count * (hash ? 4 : 1));
  for (size_t i = 0; i < count; i++) {
    const uintptr_t c = (uintptr_t)circuits_dev[i];
    ZKP_REQUIRE(c != 0, ZKP_ERR_BAD_ARG);
    require_aligned16(circuits_dev[i]);
    spans.push_back({c, c + (2 * n - 2) * 32, true});
    if (!hash) continue;
    const uintptr_t v = (uintptr_t)val_dev[i], a = (uintptr_t)addr_dev[i], t = (uintptr_t)ts_dev[i];
    ZKP_REQUIRE(v && (a & 3) == 0 && (t & 3) == 0 && ts_add[i] <= 1, ZKP_ERR_BAD_ARG);
    require_aligned16(val_dev[i]);
    spans.push_back({v, v + n * 32, false});
    if (a) spans.push_back({a, a + n * 4, false});
    if (t) spans.push_back({t, t + n * 4, false});
  }
  require_disjoint_outputs(std::move(spans));

  // groups: entries with the same (addr, val, ts) and different ts_add share one hash
  std::vector<SpGroup> groups;
  if (hash) {
    groups.reserve(count);
    for (size_t i = 0; i < count; i++) {
      const uint32_t* a = addr_dev[i];
      const uint32_t* v = reinterpret_cast<const uint32_t*>(val_dev[i]);
      const uint32_t* t = ts_dev[i];
      SpGroup* g = nullptr;
      for (SpGroup& c : groups)
        if (c.addr == a && c.val == v && c.ts == t && !c.out[ts_add[i]]) {
          g = &c;
          break;
        }
      if (!g) {
        groups.push_back(SpGroup{a, v, t, {nullptr, nullptr}, {0, 0}});
        g = &groups.back();
      }
      g->out[ts_add[i]] = reinterpret_cast<uint32_t*>(circuits_dev[i]);
      g->idx[ts_add[i]] = (uint32_t)i;
    }
  }
  hostf::FrE r2e{};
  memcpy(r2e.data(), fr.r2, 32);
  const hostf::FrE g1sq_r = fr.mul(fr.mul(g1, g1), r2e);          // (gamma1^2 R) R: the Montgomery word of gamma1^2 R
  with_fr(curve, [&](auto tag) {
    using A = FrArg<Fp<decltype(tag)>>;
    circuits_t<decltype(tag)>(ctx, groups, count, circuits_dev, n, {A(g1sq_r.data()), A(g1.data()), A(g2.data())}, roots_host);
  });
}

}  // namespace zkp
