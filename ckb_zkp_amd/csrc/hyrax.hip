// Hyrax's data-parallel GKR (hyrax/src/hyrax_proof.rs:92-147, zk_sumcheck_proof.rs:83-224): n copies of one layered circuit, the
// table work of the sum-check over the copy variables (sumcheck #1) and the evaluation of a layer over all copies.  Fr only, so one
// object serves both curves.  Sum-checks #2 and #3 (:241-442) are Libra's two phases on the tables of gkr.hip.
//
// Layout.  A layer over all copies is node-major: V[i n + t] is node i in copy t.  Consecutive lanes walk consecutive copies: every
// load is coalesced, and the gate entry and its weight are the same for a whole wavefront.
//
// The per-gate table of the reference (temp_vec, :89-95) is rank one, temp_vec[g][t] = w[g] eq[t], and combine_with_r keeps it so:
// the round polynomial is g(X) = sum_j eq_X[j] sum_g w[g] op_g(L_X[j], R_X[j]) with every table at lo + X (hi - lo).
//
// Evaluate.  Thread = column j, the gates grouped by their left node (side[0] of the layer).  Per node the thread loads L once.  A
// mul gate adds a0 += w R_lo, a1 += w dR and the node's share at X is L_X (a0 + X a1): two products per gate and three per node
// that has a mul gate.  An add gate adds b0 += w (L_lo + R_lo), b1 += w (dL + dR) for the whole chunk, whose share is b0 + X b1:
// two products and no node product.  (In natural order w (L_X R_X) and w (L_X + R_X) at three points are six and three.)
// eq_X[j] is multiplied in once per thread.  The list is cut into chunks of HYRAX_CHUNK entries (a chunk may begin and end inside
// a segment: the shares add up), one workgroup per (256 columns, chunk); one partial per workgroup and point, a small launch
// adds them.
// Bind.  One launch over (row, j) and the eq row; each position is owned by one thread.  It is not fused into the evaluation: many
// gates read one row.  The closing call gathers element 0 of every row (v_vec, :222-224) in that same launch.
// No hand-off between workgroups of one launch.  Field addition is exact: the order of a sum does not change a bit.
#include <algorithm>
#include <vector>

#include "fr_dev.hpp"
#include "hyrax.hpp"

namespace zkp {

namespace {

constexpr int HT = (int)HYRAX_THREADS;
constexpr uint32_t HYRAX_OP = 0x80000000u;

// out[g n + t] = op ? in[l n + t] in[r n + t] : in[l n + t] + in[r n + t] for g < n_gates, 0 for n_gates <= g < 2^log_out
template <class P>
__global__ __launch_bounds__(HT) void hyrax_eval_kernel(const uint2* __restrict__ nat, size_t n_gates, size_t total, int log_n,
                                                        const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  using F = Fp<P>;
  const size_t id = (size_t)blockIdx.x * HT + threadIdx.x;
  if (id >= total) return;
  const size_t g = id >> log_n, t = id & (((size_t)1 << log_n) - 1);
  F v = F::zero();
  if (g < n_gates) {
    const uint2 e = nat[g];
    const F a = F::load(in + (((size_t)e.x << log_n) + t) * 8), b = F::load(in + (((size_t)(e.y & ~HYRAX_OP) << log_n) + t) * 8);
    v = (e.y & HYRAX_OP) ? a * b : a + b;
  }
  v.store(out + id * 8);
}

// t[j] = t[j] + x (t[j + m] - t[j]) for j < m = 2^log_m, over rows 0 .. rows - 1 of v (stride n) and, as row `rows`, eq.
// finals != NULL (m == 1): finals[row] = the bound v[row n].
template <class P>
__global__ __launch_bounds__(HT) void hyrax_bind_kernel(uint32_t* __restrict__ v, uint32_t* __restrict__ eq, size_t rows, int log_n,
                                                        int log_m, FrArg<Fp<P>> xa, uint32_t* __restrict__ finals) {
  using F = Fp<P>;
  const size_t id = (size_t)blockIdx.x * HT + threadIdx.x;
  const size_t row = id >> log_m, j = id & (((size_t)1 << log_m) - 1), m = (size_t)1 << log_m;
  if (row > rows) return;
  uint32_t* t = row < rows ? v + (row << log_n) * 8 : eq;
  const F lo = F::load(t + j * 8);
  const F b = lo + xa.get() * (F::load(t + (j + m) * 8) - lo);
  b.store(t + j * 8);
  if (finals && row < rows) b.store(finals + row * 8);
}

// Workgroup blockIdx.x = k gx + c: columns [256 c, 256 c + 256) of h, entries [32 k, 32 k + 32) of the by-left-node list.
// partial[(point gridDim.x) + blockIdx.x], points X = 0, 2, 3.
template <class P>
__global__ __launch_bounds__(HT) void hyrax_round_kernel(const uint32_t* __restrict__ ptr, const uint2* __restrict__ ent, uint32_t n_gates,
                                                         uint32_t nodes, const uint32_t* __restrict__ v, const uint32_t* __restrict__ eq,
                                                         const uint32_t* __restrict__ w, int log_n, size_t h, uint32_t gx,
                                                         uint32_t* __restrict__ partial) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[3 * HT * 32];
  const uint32_t c = blockIdx.x % gx, k = blockIdx.x / gx;
  const size_t j = (size_t)c * HT + threadIdx.x;
  F e[3];
#pragma unroll
  for (int p = 0; p < 3; p++) e[p] = F::zero();
  if (j < h) {
    const uint32_t begin = k * HYRAX_CHUNK, end = min(begin + HYRAX_CHUNK, n_gates);
    uint32_t lo = 0, hi = nodes - 1;                               // the node of entry `begin`: the first x with ptr[x + 1] > begin
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (ptr[mid + 1] > begin) hi = mid;
      else lo = mid + 1;
    }
    uint32_t node = lo, i = begin;
    F b0 = F::zero(), b1 = F::zero();                              // the add gates of the whole chunk: sum w (L + R) at lo, its slope
    while (i < end) {                                              // i < end <= ptr[nodes]: a node with entries lies ahead
      const uint32_t se = min(ptr[node + 1], end);
      if (se > i) {
        const uint32_t* row = v + (((size_t)node << log_n) + j) * 8;
        F l = F::load(row);
        const F dl = F::load(row + h * 8) - l;
        F a0 = F::zero(), a1 = F::zero();                          // the node's mul gates: sum w R at lo, its slope
        bool any_mul = false;                                      // the same for every lane
        for (; i < se; i++) {
          const uint2 en = ent[i];
          const F wg = F::load(w + (size_t)en.x * 8);
          const uint32_t* rr = v + (((size_t)(en.y & ~HYRAX_OP) << log_n) + j) * 8;
          const F r0 = F::load(rr);
          const F dr = F::load(rr + h * 8) - r0;
          const bool mul = en.y & HYRAX_OP;
          const F p0 = wg * (mul ? r0 : l + r0), p1 = wg * (mul ? dr : dl + dr);
          if (mul) {
            a0 = a0 + p0;
            a1 = a1 + p1;
            any_mul = true;
          } else {
            b0 = b0 + p0;
            b1 = b1 + p1;
          }
        }
        if (any_mul) {                                             // L_X (a0 + X a1) at X = 0, 2, 3
          e[0] = e[0] + l * a0;
          l = l + dl + dl;
          a0 = a0 + a1 + a1;
          e[1] = e[1] + l * a0;
          e[2] = e[2] + (l + dl) * (a0 + a1);
        }
      }
      node++;
    }
    e[0] = e[0] + b0;
    b0 = b0 + b1 + b1;
    e[1] = e[1] + b0;
    e[2] = e[2] + b0 + b1;
    const F q0 = F::load(eq + j * 8);
    const F dq = F::load(eq + (j + h) * 8) - q0;
    const F q2 = q0 + dq + dq;
    e[0] = e[0] * q0;
    e[1] = e[1] * q2;
    e[2] = e[2] * (q2 + dq);
  }
  fr_block_sum<F, HT, 3>(e, smem);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < 3; p++) e[p].store(partial + ((size_t)p * gridDim.x + blockIdx.x) * 8);
  }
}

void require_layer(zkp_ctx* ctx, const zkp_gkr_layer* layer) {
  ZKP_REQUIRE(layer != nullptr, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(layer->device == ctx->device, ZKP_ERR_BAD_HANDLE);
}

template <class P>
void round_t(zkp_ctx* ctx, const zkp_gkr_layer* layer, uint32_t* v, uint32_t* eq, const uint32_t* w, int log_n, size_t len,
             const uint64_t* bind_host, uint64_t* evals_out_host, uint32_t* finals) {
  using F = Fp<P>;
  hipStream_t st = ctx->cur->stream;
  const size_t rows = (size_t)1 << layer->log_in;
  const size_t h = (bind_host ? len / 2 : len) / 2;               // the columns of the evaluation
  const uint32_t gx = fr_blocks(h, HT), gy = (uint32_t)((layer->n_gates + HYRAX_CHUNK - 1) / HYRAX_CHUNK), nwg = gx * gy;
  uint32_t *d_part = nullptr, *d_out = nullptr;
  if (evals_out_host) {                                            // the scratch first: growing it frees and allocates
    Scratch sc;                                                    // one partial per (point, workgroup): at most 3 * 2^20 elements
    const size_t o_part = sc.take((size_t)3 * nwg * 32), o_out = sc.take(3 * 32);
    sc.resolve(ctx->poly_tmp);
    d_part = sc.at<uint32_t>(o_part);
    d_out = sc.at<uint32_t>(o_out);
  }
  if (bind_host) {
    const size_t m = len / 2;
    hipLaunchKernelGGL(hyrax_bind_kernel<P>, dim3(fr_blocks((rows + 1) * m, HT)), dim3(HT), 0, st, v, eq, rows, log_n, log2_ceil(m),
                       FrArg<F>(bind_host), finals);
  }
  if (evals_out_host) {
    const GkrSide& sd = layer->side[0];
    hipLaunchKernelGGL(hyrax_round_kernel<P>, dim3(nwg), dim3(HT), 0, st, sd.ptr, sd.ent, (uint32_t)layer->n_gates, (uint32_t)rows, v, eq, w,
                       log_n, h, gx, d_part);
    fr_sum_partials<P, HT>(st, d_part, nwg, 3, d_out);
  }
  ZKP_HIP(hipGetLastError());
  if (evals_out_host) ZKP_HIP(hipMemcpyAsync(evals_out_host, d_out, 3 * 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

}  // namespace

void fr_gkr_eval_layer_batch(zkp_ctx* ctx, int curve, const zkp_gkr_layer* layer, const uint64_t* in_dev, uint64_t* out_dev, size_t n) {
  fr_require_curve(curve);
  require_layer(ctx, layer);
  ZKP_REQUIRE(in_dev && out_dev, ZKP_ERR_BAD_ARG);
  require_aligned16(in_dev);
  require_aligned16(out_dev);
  ZKP_REQUIRE(is_pow2(n) && n <= ((size_t)1 << HYRAX_MAX_LOG), ZKP_ERR_BAD_ARG);
  const int log_n = log2_ceil(n);
  ZKP_REQUIRE((int)layer->log_in + log_n <= HYRAX_MAX_LOG && (int)layer->log_out + log_n <= HYRAX_MAX_LOG, ZKP_ERR_BAD_ARG);
  const size_t total = ((size_t)1 << layer->log_out) * n, below = ((size_t)1 << layer->log_in) * n;
  require_disjoint_outputs({fr_span(in_dev, below, false), fr_span(out_dev, total, true)});
  hipStream_t st = ctx->cur->stream;
  with_fr(curve, [&](auto tag) {
    hipLaunchKernelGGL(hyrax_eval_kernel<decltype(tag)>, dim3(fr_blocks(total, HT)), dim3(HT), 0, st, layer->nat, (size_t)layer->n_gates, total,
                       log_n, reinterpret_cast<const uint32_t*>(in_dev), reinterpret_cast<uint32_t*>(out_dev));
  });
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipStreamSynchronize(st));
}

void fr_gkr_dp_round(zkp_ctx* ctx, int curve, const zkp_gkr_layer* layer, uint64_t* v_dev, uint64_t* eq_dev, const uint64_t* w_dev,
                     size_t n, size_t len, const uint64_t* bind_host, uint64_t* evals_out_host, uint64_t* finals_dev) {
  fr_require_curve(curve);
  require_layer(ctx, layer);
  ZKP_REQUIRE(v_dev && eq_dev && w_dev, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(bind_host || evals_out_host, ZKP_ERR_BAD_ARG);
  require_aligned16(v_dev);
  require_aligned16(eq_dev);
  require_aligned16(w_dev);
  require_aligned16(finals_dev);
  ZKP_REQUIRE(is_pow2(n) && is_pow2(len) && len <= n && n <= ((size_t)1 << HYRAX_MAX_LOG), ZKP_ERR_BAD_ARG);
  const int log_n = log2_ceil(n);
  ZKP_REQUIRE((int)layer->log_in + log_n <= HYRAX_MAX_LOG, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!bind_host || len >= 2, ZKP_ERR_BAD_ARG);
  const size_t after = bind_host ? len / 2 : len;
  ZKP_REQUIRE(!evals_out_host || after >= 2, ZKP_ERR_BAD_ARG);    // the length at evaluation time
  ZKP_REQUIRE(!finals_dev || (bind_host && after == 1), ZKP_ERR_BAD_ARG);
  if (evals_out_host) {
    const uint64_t gx = (after / 2 + HT - 1) / HT, gy = (layer->n_gates + HYRAX_CHUNK - 1) / HYRAX_CHUNK;
    ZKP_REQUIRE(gx * gy <= ((uint64_t)1 << HYRAX_MAX_LOG_WG), ZKP_ERR_BAD_ARG);
  }
  if (bind_host) fr_require_canonical(curve, bind_host, 1);
  const size_t rows = (size_t)1 << layer->log_in, total = (size_t)1 << layer->log_out;
  std::vector<MemSpan> spans = {fr_span(v_dev, rows * n, true), fr_span(eq_dev, n, true), fr_span(w_dev, total, false)};
  if (finals_dev) spans.push_back(fr_span(finals_dev, rows, true));
  require_disjoint_outputs(spans);
  with_fr(curve, [&](auto tag) {
    round_t<decltype(tag)>(ctx, layer, reinterpret_cast<uint32_t*>(v_dev), reinterpret_cast<uint32_t*>(eq_dev),
                           reinterpret_cast<const uint32_t*>(w_dev), log_n, len, bind_host, evals_out_host,
                           reinterpret_cast<uint32_t*>(finals_dev));
  });
}

}  // namespace zkp
