// Libra's linear-time GKR, the table work of one circuit layer (libra/src/libra_linear_gkr.rs:51-110 and its ZK twin): layer
// evaluation (circuit.rs:140-185), the bookkeeping tables eval_hg / eval_fgu (evaluate.rs:79-119) and the rounds of
// phase_one_prover / phase_two_prover (sumcheck.rs:21-173, 186-426).  Fr only, so one object serves both curves.
//
// Wiring.  The circuit is fixed, so the host sorts once (zkp_gkr_layer_upload): the gates in natural order, and the gates grouped
// by their left and by their right wire (counting sort: gate order within a segment).  An entry is {gate, other wire | op << 31}.
//
// Tables.  eval_hg scatters G[g] V[y] into slot x of every gate; grouped by x that is a gather: the thread that owns node x adds
// the products of its segment in registers and writes every table's slot x once, zeros included.  No atomics, one product per
// gate (an add gate's add1 term is G[g] itself).  A segment of more than GKR_LONG entries would hold its whole wavefront back, so
// the upload cuts it into chunks of GKR_CHUNK entries: one workgroup per chunk leaves a partial (fr_block_sum), one workgroup per
// long segment adds its partials.  The one-thread kernel skips those nodes: three launches that never write the same slot.
// eval_fgu is the same pass grouped by the right wire with w = eq(ru).
//
// Rounds.  g1 = f (mul + add1) + add2 and g2 = fu (mul f + add) + add f are quadratic, so a round is g(0) and g(2).  As in
// sc_round_kernel (sumcheck.hip) the bind of challenge i-1 and the evaluation of round i are ONE pass: with q = len/4 thread j < q
// owns column j of every table, binds t[j] and t[j+q] in place and evaluates from the bound values in registers.  fu is uniform:
// phase two sums mul f + add and add f separately and the final kernel combines them once per point.
// No hand-off between workgroups of one launch.  Field addition is exact: the order of a sum does not change a bit.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "fr_dev.hpp"
#include "gkr.hpp"

zkp_gkr_layer::~zkp_gkr_layer() {
  for (void* p : owned) (void)hipFree(p);
}

namespace zkp {

namespace {

constexpr int GKR_THREADS = 256;
constexpr uint32_t GKR_OP = 0x80000000u;

struct GkrPtrs {
  uint32_t* t[4];
};

__host__ __device__ constexpr int gkr_tables_of(int phase) { return phase == 1 ? 3 : 2; }   // outputs of the tables call
__host__ __device__ constexpr int gkr_round_tables(int phase) { return phase == 1 ? 4 : 3; }
__host__ __device__ constexpr int gkr_round_sums(int phase) { return phase == 1 ? 2 : 4; }  // per workgroup: points x sums per point

// out[g] = op ? in[l] in[r] : in[l] + in[r] for g < n, 0 for n <= g < total
template <class P>
__global__ __launch_bounds__(GKR_THREADS) void gkr_eval_kernel(const uint2* __restrict__ nat, size_t n, size_t total,
                                                               const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  using F = Fp<P>;
  const size_t g = (size_t)blockIdx.x * GKR_THREADS + threadIdx.x;
  if (g >= total) return;
  F v = F::zero();
  if (g < n) {
    const uint2 e = nat[g];
    const F a = F::load(in + (size_t)e.x * 8), b = F::load(in + (size_t)(e.y & ~GKR_OP) * 8);
    v = (e.y & GKR_OP) ? a * b : a + b;
  }
  v.store(out + g * 8);
}

// one entry of a segment.  Phase 1: acc = mul, add1, add2.  Phase 2: acc = mul, add.
template <class F, int PHASE>
__device__ __forceinline__ void gkr_entry(F (&acc)[gkr_tables_of(PHASE)], const uint2 e, const uint32_t* __restrict__ G,
                                          const uint32_t* __restrict__ w) {
  const F gg = F::load(G + (size_t)e.x * 8);
  const F p = gg * F::load(w + (size_t)(e.y & ~GKR_OP) * 8);
  if (e.y & GKR_OP) {
    acc[0] = acc[0] + p;
  } else if (PHASE == 1) {
    acc[1] = acc[1] + gg;
    acc[2] = acc[2] + p;
  } else {
    acc[1] = acc[1] + p;
  }
}

// one thread per node; a long segment belongs to the chunk kernels
template <class P, int PHASE>
__global__ __launch_bounds__(GKR_THREADS) void gkr_tables_kernel(const uint32_t* __restrict__ ptr, const uint2* __restrict__ ent,
                                                                 size_t nodes, const uint32_t* __restrict__ G,
                                                                 const uint32_t* __restrict__ w, GkrPtrs out) {
  using F = Fp<P>;
  constexpr int NP = gkr_tables_of(PHASE);
  const size_t node = (size_t)blockIdx.x * GKR_THREADS + threadIdx.x;
  if (node >= nodes) return;
  const uint32_t b = ptr[node], e = ptr[node + 1];
  if (e - b > GKR_LONG) return;
  F acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) acc[p] = F::zero();
  for (uint32_t i = b; i < e; i++) gkr_entry<F, PHASE>(acc, ent[i], G, w);
#pragma unroll
  for (int p = 0; p < NP; p++) acc[p].store(out.t[p] + node * 8);
}

// one workgroup per chunk of a long segment: partial[chunk][p]
template <class P, int PHASE>
__global__ __launch_bounds__(GKR_THREADS) void gkr_chunk_kernel(const GkrChunk* __restrict__ chunks, const uint2* __restrict__ ent,
                                                                const uint32_t* __restrict__ G, const uint32_t* __restrict__ w,
                                                                uint32_t* __restrict__ partial) {
  using F = Fp<P>;
  constexpr int NP = gkr_tables_of(PHASE);
  __shared__ __attribute__((aligned(16))) char smem[NP * GKR_THREADS * 32];
  const GkrChunk c = chunks[blockIdx.x];
  F acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) acc[p] = F::zero();
  for (uint32_t i = c.begin + threadIdx.x; i < c.end; i += GKR_THREADS) gkr_entry<F, PHASE>(acc, ent[i], G, w);
  fr_block_sum<F, GKR_THREADS, NP>(acc, smem);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < NP; p++) acc[p].store(partial + ((size_t)blockIdx.x * NP + p) * 8);
  }
}

// one workgroup per long segment: the sum of its chunks' partials into slot `node` of every table
template <class P, int PHASE>
__global__ __launch_bounds__(GKR_THREADS) void gkr_long_kernel(const GkrLong* __restrict__ longs, const uint32_t* __restrict__ partial,
                                                               GkrPtrs out) {
  using F = Fp<P>;
  constexpr int NP = gkr_tables_of(PHASE);
  __shared__ __attribute__((aligned(16))) char smem[NP * GKR_THREADS * 32];
  const GkrLong l = longs[blockIdx.x];
  F acc[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) acc[p] = F::zero();
  for (uint32_t c = threadIdx.x; c < l.n_chunks; c += GKR_THREADS) {
#pragma unroll
    for (int p = 0; p < NP; p++) acc[p] = acc[p] + F::load(partial + ((size_t)(l.first_chunk + c) * NP + p) * 8);
  }
  fr_block_sum<F, GKR_THREADS, NP>(acc, smem);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < NP; p++) acc[p].store(out.t[p] + (size_t)l.node * 8);
  }
}

// h threads: BIND ? len/4 : len/2.  Phase 1 tables f, mul, add1, add2: sums g(0), g(2).  Phase 2 tables f, mul, add: sums
// (mul f + add)(0), (add f)(0), (mul f + add)(2), (add f)(2).  partial[sum][workgroup].
template <class P, int PHASE, bool BIND>
__global__ __launch_bounds__(GKR_THREADS) void gkr_round_kernel(GkrPtrs tb, size_t h, FrArg<Fp<P>> xa, uint32_t* __restrict__ partial) {
  using F = Fp<P>;
  constexpr int NT = gkr_round_tables(PHASE), NS = gkr_round_sums(PHASE);
  __shared__ __attribute__((aligned(16))) char smem[NS * GKR_THREADS * 32];
  const size_t j = (size_t)blockIdx.x * GKR_THREADS + threadIdx.x;
  F e[NS];
#pragma unroll
  for (int q = 0; q < NS; q++) e[q] = F::zero();
  if (j < h) {
    const F x = xa.get();
    F lo[NT], d[NT];
#pragma unroll
    for (int s = 0; s < NT; s++) {
      uint32_t* t = tb.t[s];
      F hi;
      if (BIND) {
        const F a0 = F::load(t + j * 8), a1 = F::load(t + (j + h) * 8);
        const F b0 = F::load(t + (j + 2 * h) * 8), b1 = F::load(t + (j + 3 * h) * 8);
        lo[s] = a0 + x * (b0 - a0);
        hi = a1 + x * (b1 - a1);
        lo[s].store(t + j * 8);
        hi.store(t + (j + h) * 8);
      } else {
        lo[s] = F::load(t + j * 8);
        hi = F::load(t + (j + h) * 8);
      }
      d[s] = hi - lo[s];
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
      if (p == 1) {
#pragma unroll
        for (int s = 0; s < NT; s++) lo[s] = lo[s] + d[s] + d[s];
      }
      if (PHASE == 1) {
        e[p] = lo[0] * (lo[1] + lo[2]) + lo[3];
      } else {
        e[2 * p] = lo[1] * lo[0] + lo[2];
        e[2 * p + 1] = lo[2] * lo[0];
      }
    }
  }
  fr_block_sum<F, GKR_THREADS, NS>(e, smem);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NS; q++) e[q].store(partial + ((size_t)q * gridDim.x + blockIdx.x) * 8);
  }
}

// one workgroup per point: out[p] = sum (phase 1) or fu * sum_0 + sum_1 (phase 2) of the nwg partials
template <class P, int PHASE>
__global__ __launch_bounds__(GKR_THREADS) void gkr_final_kernel(const uint32_t* __restrict__ partial, uint32_t nwg, FrArg<Fp<P>> fua,
                                                                uint32_t* __restrict__ out) {
  using F = Fp<P>;
  constexpr int NK = gkr_round_sums(PHASE) / 2;
  __shared__ __attribute__((aligned(16))) char smem[NK * GKR_THREADS * 32];
  F acc[NK];
#pragma unroll
  for (int k = 0; k < NK; k++) acc[k] = F::zero();
  for (uint32_t c = threadIdx.x; c < nwg; c += GKR_THREADS) {
#pragma unroll
    for (int k = 0; k < NK; k++) acc[k] = acc[k] + F::load(partial + ((size_t)(blockIdx.x * NK + k) * nwg + c) * 8);
  }
  fr_block_sum<F, GKR_THREADS, NK>(acc, smem);
  if (threadIdx.x == 0) {
    if (PHASE == 1) acc[0].store(out + (size_t)blockIdx.x * 8);
    else (fua.get() * acc[0] + acc[NK - 1]).store(out + (size_t)blockIdx.x * 8);
  }
}

// t[j] = t[j] + x (t[j + m] - t[j]) for j < m, table blockIdx.y
template <class P>
__global__ __launch_bounds__(GKR_THREADS) void gkr_bind_kernel(GkrPtrs tb, size_t m, FrArg<Fp<P>> xa) {
  using F = Fp<P>;
  const size_t j = (size_t)blockIdx.x * GKR_THREADS + threadIdx.x;
  if (j >= m) return;
  const F x = xa.get();
  uint32_t* t = tb.t[blockIdx.y];
  const F lo = F::load(t + j * 8);
  (lo + x * (F::load(t + (j + m) * 8) - lo)).store(t + j * 8);
}

template <class T>
T* upload_array(zkp_gkr_layer* layer, const std::vector<T>& host) {
  if (host.empty()) return nullptr;
  void* p = nullptr;
  if (hipMalloc(&p, host.size() * sizeof(T)) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
  layer->owned.push_back(p);
  ZKP_HIP(hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
  return reinterpret_cast<T*>(p);
}

template <class P, int PHASE>
void tables_t(zkp_ctx* ctx, const zkp_gkr_layer* layer, const uint32_t* G, const uint32_t* w, const GkrPtrs& out) {
  constexpr int NP = gkr_tables_of(PHASE);
  const GkrSide& sd = layer->side[PHASE - 1];
  const size_t nodes = (size_t)1 << layer->log_in;
  hipStream_t st = ctx->cur->stream;
  // the scratch first: growing it frees and allocates, which would come between the launches
  uint32_t* partial = sd.n_long ? ctx->poly_tmp.as<uint32_t>((size_t)sd.n_chunks * NP * 8) : nullptr;
  hipLaunchKernelGGL((gkr_tables_kernel<P, PHASE>), dim3(fr_blocks(nodes, GKR_THREADS)), dim3(GKR_THREADS), 0, st, sd.ptr, sd.ent, nodes, G, w, out);
  if (sd.n_long) {
    hipLaunchKernelGGL((gkr_chunk_kernel<P, PHASE>), dim3(sd.n_chunks), dim3(GKR_THREADS), 0, st, sd.chunks, sd.ent, G, w, partial);
    hipLaunchKernelGGL((gkr_long_kernel<P, PHASE>), dim3(sd.n_long), dim3(GKR_THREADS), 0, st, sd.longs, partial, out);
  }
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipStreamSynchronize(st));
}

template <class P, int PHASE>
void round_t(zkp_ctx* ctx, const GkrPtrs& tb, size_t len, const uint64_t* fu_host, const uint64_t* bind_host, uint64_t* evals_out_host) {
  using F = Fp<P>;
  constexpr int NT = gkr_round_tables(PHASE), NS = gkr_round_sums(PHASE);
  hipStream_t st = ctx->cur->stream;
  const FrArg<F> xa(bind_host);
  if (!evals_out_host) {                                         // bind only
    const size_t m = len / 2;
    hipLaunchKernelGGL(gkr_bind_kernel<P>, dim3(fr_blocks(m, GKR_THREADS), NT), dim3(GKR_THREADS), 0, st, tb, m, xa);
    ZKP_HIP(hipGetLastError());
    ZKP_HIP(hipStreamSynchronize(st));
    return;
  }
  const size_t h = bind_host ? len / 4 : len / 2;
  const uint32_t nwg = fr_blocks(h, GKR_THREADS);
  Scratch sc;                                                    // one partial per (sum, workgroup): at most 4 * 2^19 elements
  const size_t o_part = sc.take((size_t)NS * nwg * 32), o_out = sc.take(2 * 32);
  sc.resolve(ctx->poly_tmp);
  uint32_t* d_part = sc.at<uint32_t>(o_part);
  uint32_t* d_out = sc.at<uint32_t>(o_out);
  if (bind_host) hipLaunchKernelGGL((gkr_round_kernel<P, PHASE, true>), dim3(nwg), dim3(GKR_THREADS), 0, st, tb, h, xa, d_part);
  else hipLaunchKernelGGL((gkr_round_kernel<P, PHASE, false>), dim3(nwg), dim3(GKR_THREADS), 0, st, tb, h, xa, d_part);
  hipLaunchKernelGGL((gkr_final_kernel<P, PHASE>), dim3(2), dim3(GKR_THREADS), 0, st, d_part, nwg, FrArg<F>(fu_host), d_out);
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipMemcpyAsync(evals_out_host, d_out, 2 * 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

void require_layer(zkp_ctx* ctx, const zkp_gkr_layer* layer) {
  ZKP_REQUIRE(layer != nullptr, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(layer->device == ctx->device, ZKP_ERR_BAD_HANDLE);
}

}  // namespace

zkp_gkr_layer* gkr_layer_upload(zkp_ctx* ctx, const uint8_t* op, const uint32_t* left, const uint32_t* right, size_t n_gates,
                                uint32_t log_in) {
  ZKP_REQUIRE(op && left && right, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(n_gates >= 1 && n_gates <= ((size_t)1 << GKR_MAX_LOG) && log_in <= (uint32_t)GKR_MAX_LOG, ZKP_ERR_BAD_ARG);
  const size_t nodes = (size_t)1 << log_in;
  uint64_t n_mul = 0;
  for (size_t g = 0; g < n_gates; g++) {
    ZKP_REQUIRE(op[g] <= 1 && left[g] < nodes && right[g] < nodes, ZKP_ERR_BAD_ARG);   // IllegalOperator / IllegalNode
    n_mul += op[g];
  }
  std::unique_ptr<zkp_gkr_layer> layer(new zkp_gkr_layer);
  layer->device = ctx->device;
  layer->n_gates = n_gates;
  layer->n_mul = n_mul;
  layer->log_in = log_in;
  while (((size_t)1 << layer->log_out) < n_gates) layer->log_out++;
  {
    std::vector<uint2> nat(n_gates);
    for (size_t g = 0; g < n_gates; g++) nat[g] = make_uint2(left[g], right[g] | (op[g] ? GKR_OP : 0u));
    layer->nat = upload_array(layer.get(), nat);
  }
  for (int s = 0; s < 2; s++) {
    const uint32_t* key = s ? right : left;
    const uint32_t* other = s ? left : right;
    GkrSide& sd = layer->side[s];
    std::vector<uint32_t> ptr(nodes + 1, 0);
    for (size_t g = 0; g < n_gates; g++) ptr[key[g] + 1]++;
    for (size_t v = 0; v < nodes; v++) ptr[v + 1] += ptr[v];
    std::vector<uint2> ent(n_gates);
    {
      std::vector<uint32_t> fill(ptr.begin(), ptr.end() - 1);
      for (size_t g = 0; g < n_gates; g++) ent[fill[key[g]]++] = make_uint2((uint32_t)g, other[g] | (op[g] ? GKR_OP : 0u));
    }
    std::vector<GkrLong> longs;
    std::vector<GkrChunk> chunks;
    for (size_t v = 0; v < nodes; v++) {
      const uint32_t fan = ptr[v + 1] - ptr[v];
      sd.max_fan = std::max(sd.max_fan, fan);
      if (fan <= GKR_LONG) continue;
      longs.push_back({(uint32_t)v, (uint32_t)chunks.size(), (fan + GKR_CHUNK - 1) / GKR_CHUNK});
      for (uint32_t b = ptr[v]; b < ptr[v + 1]; b += GKR_CHUNK) chunks.push_back({b, std::min(b + GKR_CHUNK, ptr[v + 1])});
    }
    sd.n_long = (uint32_t)longs.size();
    sd.n_chunks = (uint32_t)chunks.size();
    sd.ptr = upload_array(layer.get(), ptr);
    sd.ent = upload_array(layer.get(), ent);
    sd.longs = upload_array(layer.get(), longs);
    sd.chunks = upload_array(layer.get(), chunks);
  }
  return layer.release();
}

void gkr_layer_free(zkp_ctx* ctx, zkp_gkr_layer* layer) {
  require_layer(ctx, layer);
  ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));
  delete layer;
}

void gkr_layer_info(const zkp_gkr_layer* layer, uint64_t info[8]) {
  info[0] = layer->n_gates;
  info[1] = layer->log_out;
  info[2] = layer->log_in;
  info[3] = layer->n_mul;
  info[4] = layer->side[0].max_fan;
  info[5] = layer->side[1].max_fan;
  info[6] = layer->side[0].n_long;
  info[7] = layer->side[1].n_long;
}

void fr_gkr_eval_layer(zkp_ctx* ctx, int curve, const zkp_gkr_layer* layer, const uint64_t* in_dev, uint64_t* out_dev) {
  fr_require_curve(curve);
  require_layer(ctx, layer);
  ZKP_REQUIRE(in_dev && out_dev, ZKP_ERR_BAD_ARG);
  require_aligned16(in_dev);
  require_aligned16(out_dev);
  const size_t total = (size_t)1 << layer->log_out, nodes = (size_t)1 << layer->log_in;
  require_disjoint_outputs({fr_span(in_dev, nodes, false), fr_span(out_dev, total, true)});
  hipStream_t st = ctx->cur->stream;
  with_fr(curve, [&](auto tag) {
    hipLaunchKernelGGL(gkr_eval_kernel<decltype(tag)>, dim3(fr_blocks(total, GKR_THREADS)), dim3(GKR_THREADS), 0, st, layer->nat, (size_t)layer->n_gates,
                       total, reinterpret_cast<const uint32_t*>(in_dev), reinterpret_cast<uint32_t*>(out_dev));
  });
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipStreamSynchronize(st));
}

void fr_gkr_tables(zkp_ctx* ctx, int curve, const zkp_gkr_layer* layer, int phase, const uint64_t* g_dev, const uint64_t* w_dev,
                   uint64_t* const* out_dev) {
  fr_require_curve(curve);
  require_layer(ctx, layer);
  ZKP_REQUIRE(phase == 1 || phase == 2, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(g_dev && w_dev && out_dev, ZKP_ERR_BAD_ARG);
  require_aligned16(g_dev);
  require_aligned16(w_dev);
  const size_t total = (size_t)1 << layer->log_out, nodes = (size_t)1 << layer->log_in;
  const int np = gkr_tables_of(phase);
  ZKP_REQUIRE(phase == 1 || out_dev[2] == nullptr, ZKP_ERR_BAD_ARG);
  std::vector<MemSpan> spans = {fr_span(g_dev, total, false), fr_span(w_dev, nodes, false)};
  GkrPtrs out{};
  for (int p = 0; p < np; p++) {
    ZKP_REQUIRE(out_dev[p] != nullptr, ZKP_ERR_BAD_ARG);
    require_aligned16(out_dev[p]);
    spans.push_back(fr_span(out_dev[p], nodes, true));
    out.t[p] = reinterpret_cast<uint32_t*>(out_dev[p]);
  }
  require_disjoint_outputs(spans);
  const uint32_t* G = reinterpret_cast<const uint32_t*>(g_dev);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(w_dev);
  with_fr(curve, [&](auto tag) {
    if (phase == 1) tables_t<decltype(tag), 1>(ctx, layer, G, w, out);
    else tables_t<decltype(tag), 2>(ctx, layer, G, w, out);
  });
}

void fr_gkr_round(zkp_ctx* ctx, int curve, int phase, uint64_t* const* tables_dev, size_t len, const uint64_t* fu_host,
                  const uint64_t* bind_host, uint64_t* evals_out_host) {
  fr_require_curve(curve);
  ZKP_REQUIRE(phase == 1 || phase == 2, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(tables_dev != nullptr, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(bind_host || evals_out_host, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(is_pow2(len) && len <= ((size_t)1 << GKR_MAX_LOG), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!bind_host || len >= 2, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!evals_out_host || (bind_host ? len / 2 : len) >= 2, ZKP_ERR_BAD_ARG);   // the length at evaluation time
  ZKP_REQUIRE(phase == 1 || !evals_out_host || fu_host, ZKP_ERR_BAD_ARG);
  if (bind_host) fr_require_canonical(curve, bind_host, 1);
  if (phase == 2 && fu_host) fr_require_canonical(curve, fu_host, 1);
  const int nt = gkr_round_tables(phase);
  GkrPtrs tb{};
  std::vector<uintptr_t> at(nt);
  for (int s = 0; s < nt; s++) {
    ZKP_REQUIRE(tables_dev[s] != nullptr, ZKP_ERR_BAD_ARG);
    require_aligned16(tables_dev[s]);
    at[s] = (uintptr_t)tables_dev[s];
    tb.t[s] = reinterpret_cast<uint32_t*>(tables_dev[s]);
  }
  std::sort(at.begin(), at.end());                               // every table is bound in place: no two may overlap
  for (int s = 1; s < nt; s++) ZKP_REQUIRE(at[s] - at[s - 1] >= len * 32, ZKP_ERR_BAD_ARG);
  with_fr(curve, [&](auto tag) {
    if (phase == 1) round_t<decltype(tag), 1>(ctx, tb, len, nullptr, bind_host, evals_out_host);
    else round_t<decltype(tag), 2>(ctx, tb, len, fu_host, bind_host, evals_out_host);
  });
}

}  // namespace zkp
