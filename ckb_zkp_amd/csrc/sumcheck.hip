// Sum-check over dense multilinear tables of Fr (zkp_fr_sumcheck_round_dev) and eq tables (zkp_fr_eq_evals_dev): the loop of
// sum_check_proof_phase_one / _phase_two / sum_check_cubic_prover (spartan/src/prover.rs:422-592, 594-723, 1442-1607) between
// the commitments.  Fr only, so one object serves both curves (Bn254Fr / Bls381Fr).
//
// One round of the reference is combine_with_n at 2 and 3 over every table, two or three inner sums, then combine_with_r over
// every table (polynomial.rs:121-138): about ten passes.  Here the bind of challenge i-1 and the evaluation of round i are ONE
// pass.  With q = len/4, thread j < q owns column j of every table of its terms: it reads t[j], t[j+q], t[j+2q], t[j+3q], binds
//   new[j] = t[j] + x (t[j+2q] - t[j])      new[j+q] = t[j+q] + x (t[j+3q] - t[j+q])          (x hi + (1 - x) lo, canonical)
// writes both in place and adds g(lo + t (hi - lo)) with lo = new[j], hi = new[j+q] to its sums for t = 0, 2, (3).  The four
// positions of a column belong to that thread alone, so in-place binding is race-free.  A table that several terms (or several
// slots of one term) share is bound by the first slot that reaches it in the thread's own order; the later ones read the two bound
// values back (same thread, same addresses: program order).  Terms are spread over grid.y by groups that share no table.
//
// Reduction: fr_block_sum (fr_dev.hpp) leaves one partial per (workgroup, term, point); fr_sum_partials (one workgroup per
// (term, point)) adds them.  No hand-off between workgroups of one launch.  Field addition is exact: the order does not matter.
//
// Without a bind (round 0) the same kernel runs with one thread per j < len/2; a bind without evaluation (after the last round)
// is sc_bind_kernel, one thread per (table, j < len/2).
//
// eq table: thread t owns the 8 consecutive entries [8t, 8t + 8): the product over the k - 3 leading variables from the bits of
// t, then three doubling steps in registers (e -> (e - e r, e r)): (k + 4) / 8 products per entry, one launch, 16-byte stores.
#include <algorithm>
#include <cstring>
#include <vector>

#include "fr_dev.hpp"
#include "sumcheck.hpp"

namespace zkp {

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_EQ_LOW = 3;              // variables expanded in registers by the eq kernel

__host__ __device__ constexpr int sc_arity(int kind) { return kind == ZKP_SC_EQ_AB_MINUS_C ? 4 : kind == ZKP_SC_PROD2 ? 2 : 3; }
__host__ __device__ constexpr int sc_points(int kind) { return kind == ZKP_SC_PROD2 ? 2 : 3; }

struct ScTerm {
  uint32_t* t[4];
  uint32_t fresh;            // bit s: slot s is the first use of its table in this group's order (it binds and writes the table)
  uint32_t out;              // index of the term as the caller counts it
};
struct ScGroup {
  uint32_t first, n;         // terms [first, first + n) of the group-ordered term list
};

// h threads along x: BIND ? len/4 : len/2.  Tables may alias each other (shared tables), so no pointer is __restrict__.
template <class P, int KIND, bool BIND>
__global__ __launch_bounds__(SC_THREADS) void sc_round_kernel(const ScTerm* terms, const ScGroup* groups, size_t h, FrArg<Fp<P>> xa,
                                                              uint32_t* partial) {
  using F = Fp<P>;
  constexpr int AR = sc_arity(KIND), NP = sc_points(KIND);
  __shared__ __attribute__((aligned(16))) char smem[NP * SC_THREADS * 32];
  const size_t j = (size_t)blockIdx.x * SC_THREADS + threadIdx.x;
  const bool act = j < h;
  const ScGroup g = groups[blockIdx.y];
  const F x = xa.get();
  for (uint32_t k = 0; k < g.n; k++) {
    const ScTerm tm = terms[g.first + k];
    F e[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) e[p] = F::zero();
    if (act) {
      F lo[AR], d[AR];
#pragma unroll
      for (int s = 0; s < AR; s++) {
        uint32_t* t = tm.t[s];
        F hi;
        if (BIND && ((tm.fresh >> s) & 1u)) {
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
      // point 0, then 2 and 3 by stepping every table from hi = lo + d
#pragma unroll
      for (int p = 0; p < NP; p++) {
        if (p == 1) {
#pragma unroll
          for (int s = 0; s < AR; s++) lo[s] = lo[s] + d[s] + d[s];
        } else if (p == 2) {
#pragma unroll
          for (int s = 0; s < AR; s++) lo[s] = lo[s] + d[s];
        }
        if (KIND == ZKP_SC_EQ_AB_MINUS_C) e[p] = lo[0] * (lo[1] * lo[2] - lo[3]);
        else if (KIND == ZKP_SC_PROD2) e[p] = lo[0] * lo[1];
        else e[p] = lo[0] * lo[1] * lo[2];
      }
    }
    fr_block_sum<F, SC_THREADS, NP>(e, smem);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int p = 0; p < NP; p++) e[p].store(partial + ((size_t)(tm.out * NP + p) * gridDim.x + blockIdx.x) * 8);
    }
  }
}

// t[j] = t[j] + x (t[j + m] - t[j]) for j < m, table blockIdx.y
template <class P>
__global__ __launch_bounds__(SC_THREADS) void sc_bind_kernel(uint32_t* const* __restrict__ tables, size_t m, FrArg<Fp<P>> xa) {
  using F = Fp<P>;
  const size_t j = (size_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (j >= m) return;
  const F x = xa.get();
  uint32_t* t = tables[blockIdx.y];
  const F lo = F::load(t + j * 8);
  (lo + x * (F::load(t + (j + m) * 8) - lo)).store(t + j * 8);
}

// LOW variables in registers: thread t writes out[t << LOW .. (t + 1) << LOW); r: k elements, device memory
template <class P, int LOW>
__global__ __launch_bounds__(SC_THREADS) void sc_eq_kernel(const uint32_t* __restrict__ r, uint32_t k, size_t threads,
                                                           uint32_t* __restrict__ out) {
  using F = Fp<P>;
  const size_t t = (size_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (t >= threads) return;
  const uint32_t kh = k - LOW;                                   // leading variables: bit (kh - 1 - i) of t selects r[i]
  F e[1 << LOW];
  e[0] = F::one();
  for (uint32_t i = 0; i < kh; i++) {
    const F ri = F::load(r + (size_t)i * 8);
    e[0] = e[0] * (((t >> (kh - 1 - i)) & 1) ? ri : F::one() - ri);
  }
#pragma unroll
  for (int l = 0; l < LOW; l++) {
    const F rl = F::load(r + (size_t)(kh + l) * 8);
#pragma unroll
    for (int a = (1 << l) - 1; a >= 0; a--) {
      const F hi = e[a] * rl;
      e[2 * a] = e[a] - hi;
      e[2 * a + 1] = hi;
    }
  }
#pragma unroll
  for (int a = 0; a < (1 << LOW); a++) e[a].store(out + ((t << LOW) + a) * 8);
}

template <class P, int KIND>
void launch_round(hipStream_t st, bool bind, dim3 grid, const ScTerm* terms, const ScGroup* groups, size_t h, const uint64_t* x,
                  uint32_t* partial) {
  const FrArg<Fp<P>> xa(x);
  if (bind) hipLaunchKernelGGL((sc_round_kernel<P, KIND, true>), grid, dim3(SC_THREADS), 0, st, terms, groups, h, xa, partial);
  else hipLaunchKernelGGL((sc_round_kernel<P, KIND, false>), grid, dim3(SC_THREADS), 0, st, terms, groups, h, xa, partial);
}

template <class P>
void round_t(zkp_ctx* ctx, int kind, size_t count, uint64_t* const* tables, size_t len, const uint64_t* bind_host,
             uint64_t* evals_out_host) {
  const int ar = sc_arity(kind), np = sc_points(kind);
  const size_t slots = count * ar;
  // distinct tables, sorted by address: neighbours are the only candidates for an overlap (every table has len elements)
  std::vector<uintptr_t> uniq(slots);
  for (size_t i = 0; i < slots; i++) {
    ZKP_REQUIRE(tables[i] != nullptr, ZKP_ERR_BAD_ARG);
    require_aligned16(tables[i]);
    uniq[i] = (uintptr_t)tables[i];
  }
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  for (size_t i = 1; i < uniq.size(); i++) ZKP_REQUIRE(uniq[i] - uniq[i - 1] >= len * 32, ZKP_ERR_BAD_ARG);
  auto table_id = [&](const uint64_t* p) { return (size_t)(std::lower_bound(uniq.begin(), uniq.end(), (uintptr_t)p) - uniq.begin()); };
  hipStream_t st = ctx->cur->stream;

  if (!evals_out_host) {                                         // bind only
    const size_t m = len / 2;
    uint32_t** d_tab = reinterpret_cast<uint32_t**>(ctx->poly_tmp.get(uniq.size() * sizeof(uint32_t*)));
    ZKP_HIP(hipMemcpyAsync(d_tab, uniq.data(), uniq.size() * sizeof(uint32_t*), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sc_bind_kernel<P>, dim3(fr_blocks(m, SC_THREADS), (unsigned)uniq.size()), dim3(SC_THREADS),
                       0, st, d_tab, m, FrArg<Fp<P>>(bind_host));
    ZKP_HIP(hipGetLastError());
    ZKP_HIP(hipStreamSynchronize(st));
    return;
  }

  // groups: terms connected through shared tables (union-find over table ids); a group runs in one grid.y slice
  std::vector<uint32_t> parent(count), owner(uniq.size(), UINT32_MAX);
  for (size_t k = 0; k < count; k++) parent[k] = (uint32_t)k;
  auto find = [&](uint32_t a) {
    while (parent[a] != a) a = parent[a] = parent[parent[a]];
    return a;
  };
  for (size_t k = 0; k < count; k++)
    for (int s = 0; s < ar; s++) {
      uint32_t& o = owner[table_id(tables[k * ar + s])];
      if (o == UINT32_MAX) o = (uint32_t)k;
      else parent[find((uint32_t)k)] = find(o);
    }
  std::vector<uint32_t> order(count);
  for (size_t k = 0; k < count; k++) order[k] = (uint32_t)k;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return find(a) < find(b); });
  std::vector<ScTerm> terms(count);
  std::vector<ScGroup> groups;
  std::vector<uint8_t> seen(uniq.size(), 0);
  for (size_t i = 0; i < count; i++) {
    const uint32_t k = order[i];
    if (i == 0 || find(order[i - 1]) != find(k)) groups.push_back({(uint32_t)i, 0});
    groups.back().n++;
    ScTerm& tm = terms[i];
    memset(&tm, 0, sizeof tm);
    tm.out = k;
    for (int s = 0; s < ar; s++) {
      tm.t[s] = reinterpret_cast<uint32_t*>(tables[k * ar + s]);
      uint8_t& sn = seen[table_id(tables[k * ar + s])];
      if (!sn) tm.fresh |= 1u << s;
      sn = 1;
    }
  }

  const size_t h = bind_host ? len / 4 : len / 2;
  const uint32_t nwg = fr_blocks(h, SC_THREADS);
  const size_t nout = count * np;
  // one partial per (workgroup, term, point): count * points * len / 16 (len / 32 with a bind) bytes, e.g. 6 MB for one fused
  // phase-one term of 2^26 rows.  Many terms over very long tables (256 terms of 2^28 rows: 13 GB) end as ZKP_ERR_OOM, as zkp_accel.h says.
  // A loop over several columns per thread would bound this, but took the fused kernel from 139 to 229 VGPRs (occupancy 3 -> 2).
  Scratch sc;
  const size_t o_terms = sc.take(count * sizeof(ScTerm)), o_groups = sc.take(groups.size() * sizeof(ScGroup));
  const size_t o_part = sc.take(nout * nwg * 32), o_out = sc.take(nout * 32);
  sc.resolve(ctx->poly_tmp);
  ScTerm* d_terms = sc.at<ScTerm>(o_terms);
  ScGroup* d_groups = sc.at<ScGroup>(o_groups);
  uint32_t* d_part = sc.at<uint32_t>(o_part);
  uint32_t* d_out = sc.at<uint32_t>(o_out);
  ZKP_HIP(hipMemcpyAsync(d_terms, terms.data(), count * sizeof(ScTerm), hipMemcpyHostToDevice, st));
  ZKP_HIP(hipMemcpyAsync(d_groups, groups.data(), groups.size() * sizeof(ScGroup), hipMemcpyHostToDevice, st));
  const dim3 grid(nwg, (unsigned)groups.size());
  if (kind == ZKP_SC_EQ_AB_MINUS_C) launch_round<P, ZKP_SC_EQ_AB_MINUS_C>(st, bind_host != nullptr, grid, d_terms, d_groups, h, bind_host, d_part);
  else if (kind == ZKP_SC_PROD2) launch_round<P, ZKP_SC_PROD2>(st, bind_host != nullptr, grid, d_terms, d_groups, h, bind_host, d_part);
  else launch_round<P, ZKP_SC_PROD3>(st, bind_host != nullptr, grid, d_terms, d_groups, h, bind_host, d_part);
  fr_sum_partials<P, SC_THREADS>(st, d_part, nwg, (uint32_t)nout, d_out);
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipMemcpyAsync(evals_out_host, d_out, nout * 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

template <class P>
void eq_t(zkp_ctx* ctx, const uint64_t* r_host, size_t k, uint32_t* out) {
  hipStream_t st = ctx->cur->stream;
  uint32_t* rd = ctx->poly_tmp.as<uint32_t>((size_t)(SC_MAX_LOG + 1) * 8);
  if (k) ZKP_HIP(hipMemcpyAsync(rd, r_host, k * 32, hipMemcpyHostToDevice, st));
  if (k >= SC_EQ_LOW) {
    const size_t threads = (size_t)1 << (k - SC_EQ_LOW);
    hipLaunchKernelGGL((sc_eq_kernel<P, SC_EQ_LOW>), dim3(fr_blocks(threads, SC_THREADS)), dim3(SC_THREADS), 0, st,
                       rd, (uint32_t)k, threads, out);
  } else {
    hipLaunchKernelGGL((sc_eq_kernel<P, 0>), dim3(1), dim3(SC_THREADS), 0, st, rd, (uint32_t)k, (size_t)1 << k, out);
  }
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipStreamSynchronize(st));                             // r_host and the staging area are free again
}

}  // namespace

void fr_sumcheck_round(zkp_ctx* ctx, int curve, int kind, size_t count, uint64_t* const* tables, size_t len, const uint64_t* bind_host,
                       uint64_t* evals_out_host) {
  fr_require_curve(curve);
  ZKP_REQUIRE(kind == ZKP_SC_EQ_AB_MINUS_C || kind == ZKP_SC_PROD2 || kind == ZKP_SC_PROD3, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(bind_host || evals_out_host, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(count <= SC_MAX_TERMS, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(is_pow2(len) && len <= ((size_t)1 << SC_MAX_LOG), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!bind_host || len >= 2, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!evals_out_host || (bind_host ? len / 2 : len) >= 2, ZKP_ERR_BAD_ARG);   // the length at evaluation time
  if (bind_host) fr_require_canonical(curve, bind_host, 1);
  if (count == 0) return;
  ZKP_REQUIRE(tables != nullptr, ZKP_ERR_BAD_ARG);
  with_fr(curve, [&](auto tag) { round_t<decltype(tag)>(ctx, kind, count, tables, len, bind_host, evals_out_host); });
}

void fr_eq_evals(zkp_ctx* ctx, int curve, const uint64_t* r_host, size_t k, uint64_t* out_dev) {
  fr_require_curve(curve);
  ZKP_REQUIRE(k <= (size_t)SC_MAX_LOG, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(out_dev && (k == 0 || r_host), ZKP_ERR_BAD_ARG);
  require_aligned16(out_dev);
  fr_require_canonical(curve, r_host, k);
  with_fr(curve, [&](auto tag) { eq_t<decltype(tag)>(ctx, r_host, k, reinterpret_cast<uint32_t*>(out_dev)); });
}

}  // namespace zkp
