// Marlin prover behind the C ABI: the host-side orchestration of
//   /root/reference/marlin/src/lib.rs:97-181            create_random_proof (round -> PC::commit -> absorb -> squeeze)
//   /root/reference/marlin/src/ahp/indexer.rs:70-117    AHP::index — the device half: compose_matrix_polynomials
//   /root/reference/marlin/src/ahp/arithmetic.rs:98-172   (row / col / val / row_col over K, interpolation, evaluation over B)
//   /root/reference/marlin/src/ahp/prover.rs:86-427     prover_init, prover_{first,second,third}_round
//   /root/reference/marlin/src/pc/mod.rs:34-160         PC::commit, open, batch_open over KZG10 (pc/kzg10.rs:100-156)
// over the device primitives of this library (NTTs, element-wise Fr kernels, batch inversion, sparse products, gathers,
// vanishing-polynomial folds, Horner evaluation / division, MSMs on the resident SRS powers).  Every vector stays in HBM;
// the host handles scalars: the verifier messages (FiatShamirRng, fs_rng.cpp), a handful of mask coefficients and the
// 32-byte read-backs of evaluations and commitments.  No arithmetic kernels live here.
//
// What stays on the caller's side (Rust): circuit synthesis, make_matrices_square / balance_matrices / the per-row column
// sort of AHP::index (pure index manipulation, ahp/constraint_systems.rs:9-31,100-133), and the zk RNG: the mask
// coefficients and commitment blinders are inputs (`zkp_marlin_rand`).
#include <algorithm>
#include <chrono>
#include <array>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "fr_dev.hpp"
#include "host_field.hpp"
#include "internal.hpp"
#include "msm_vtbl.hpp"

// fs_rng.cpp (C ABI, same library)
extern "C" {
int32_t zkp_fs_rng_new(const uint8_t*, size_t, zkp_fs_rng**);
int32_t zkp_fs_rng_free(zkp_fs_rng*);
int32_t zkp_fs_rng_absorb(zkp_fs_rng*, const uint8_t*, size_t);
int32_t zkp_fs_rng_rand_u128(zkp_fs_rng*, uint64_t[2]);
int32_t zkp_fs_rng_rand_fr(zkp_fs_rng*, zkp_curve_t, uint64_t*);
int32_t zkp_fs_rng_sample_outside_domain(zkp_fs_rng*, zkp_curve_t, uint32_t, uint64_t*);
}

namespace zkp {
namespace {

using namespace hostf;

size_t next_pow2(size_t n) {
  size_t s = 1;
  while (s < n) s <<= 1;
  return s;
}

// ------------------------------------------------------------------------------------------------ device vectors
struct DVec {
  uint64_t* p = nullptr;   // device, Fr Montgomery
  size_t n = 0;
  DVec view(size_t a, size_t b) const { return DVec{p + 4 * a, b - a}; }
  DVec view(size_t a) const { return view(a, n); }
};

// size-keyed free lists: a proof allocates the same ~120 vectors every time, so after the first proof no hipMalloc / hipFree
// (each a device-wide synchronisation) is left in the path; reuse is stream-ordered (one stream)
struct Pool {
  std::map<size_t, std::vector<void*>> free_;
  std::vector<std::pair<void*, size_t>> live;
  void* raw(size_t bytes) {
    bytes = std::max<size_t>(bytes, 32);
    auto& f = free_[bytes];
    void* p = nullptr;
    if (!f.empty()) {
      p = f.back();
      f.pop_back();
    } else if (hipMalloc(&p, bytes) != hipSuccess) {
      throw StatusError{ZKP_ERR_OOM};
    }
    live.push_back({p, bytes});
    return p;
  }
  void release_all() {
    for (auto& l : live) free_[l.second].push_back(l.first);
    live.clear();
  }
  void trim() {
    release_all();
    for (auto& kv : free_)
      for (void* p : kv.second) (void)hipFree(p);
    free_.clear();
  }
};

struct Backend {
  zkp_ctx* ctx;
  int curve;
  HostField F;
  Pool* pool;
  hipStream_t st() const { return ctx->cur->stream; }
  DVec alloc(size_t n) { return DVec{reinterpret_cast<uint64_t*>(pool->raw(std::max<size_t>(n, 1) * 32)), n}; }
  DVec zeros(size_t n) {
    DVec v = alloc(n);
    if (n) ZKP_HIP(hipMemsetAsync(v.p, 0, n * 32, st()));
    return v;
  }
  DVec upload(const uint64_t* host_mont, size_t n) {
    DVec v = alloc(n);
    if (n) ZKP_HIP(hipMemcpyAsync(v.p, host_mont, n * 32, hipMemcpyHostToDevice, st()));
    return v;
  }
  DVec upload(const std::vector<FrE>& els) {
    std::vector<uint64_t> h(els.size() * 4 + 4);
    for (size_t i = 0; i < els.size(); i++) memcpy(&h[4 * i], els[i].data(), 32);
    DVec v = alloc(els.size());
    if (!els.empty()) {
      ZKP_HIP(hipMemcpyAsync(v.p, h.data(), els.size() * 32, hipMemcpyHostToDevice, st()));
      ZKP_HIP(hipStreamSynchronize(st()));             // h dies with this call
    }
    return v;
  }
  void copy_into(DVec dst, DVec src) {
    if (src.n) ZKP_HIP(hipMemcpyAsync(dst.p, src.p, src.n * 32, hipMemcpyDeviceToDevice, st()));
  }
  DVec pad(DVec v, size_t n) {
    DVec out = zeros(n);
    copy_into(out, v.view(0, std::min(v.n, n)));
    return out;
  }
  DVec shift(DVec v, size_t s) {
    DVec out = zeros(v.n + s);
    copy_into(out.view(s), v);
    return out;
  }
  void op(int o, DVec a, const uint64_t* b, DVec out, size_t n, const FrE* k = nullptr) {
    fr_vec_op(ctx, curve, o, a.p, b, k ? reinterpret_cast<const uint64_t*>(k->data()) : nullptr, out.p, n);
  }
  DVec mul(DVec a, DVec b) {
    DVec out = alloc(a.n);
    op(ZKP_VEC_MUL, a, b.p, out, a.n);
    return out;
  }
  DVec scale(DVec a, const FrE& k) {
    DVec out = alloc(a.n);
    op(ZKP_VEC_SCALE, a, nullptr, out, a.n, &k);
    return out;
  }
  DVec addc(DVec a, const FrE& k) {
    DVec out = alloc(a.n);
    op(ZKP_VEC_ADDC, a, nullptr, out, a.n, &k);
    return out;
  }
  DVec axpy(DVec a, DVec b, const FrE& k) {            // a + k*b, zero-extended to max(len)
    DVec out = pad(a, std::max(a.n, b.n));
    op(ZKP_VEC_AXPY, out.view(0, b.n), b.p, out.view(0, b.n), b.n, &k);
    return out;
  }
  void axpy_into(DVec acc, DVec b, const FrE& k, size_t at = 0) {
    DVec t = acc.view(at, at + b.n);
    op(ZKP_VEC_AXPY, t, b.p, t, b.n, &k);
  }
  void add_at(DVec v, size_t i, const FrE& k) {
    DVec e = v.view(i, i + 1);
    op(ZKP_VEC_ADDC, e, nullptr, e, 1, &k);
  }
  DVec sub(DVec a, DVec b) { return axpy(a, b, F.neg(F.one_())); }
  DVec binv(DVec a) {
    DVec out = pad(a, a.n);
    fr_batch_inverse(ctx, curve, out.p, out.n);
    return out;
  }
  DVec ntt(DVec v, size_t size, int o) {
    DVec out = pad(v, size);
    ntt_run(ctx, curve, reinterpret_cast<uint32_t*>(out.p), log2_ceil(size), o);
    return out;
  }
  uint64_t ntt_count = 0, ntt_elements = 0;            // bookkeeping for zkp_marlin_last_timing
  DVec fft(DVec v, size_t size) {
    ntt_count++;
    ntt_elements += size;
    return ntt(v, size, ZKP_NTT_FFT);
  }
  DVec ifft(DVec v, size_t size) {
    ntt_count++;
    ntt_elements += size;
    return ntt(v, size, ZKP_NTT_IFFT);
  }
  DVec pmul(DVec a, DVec b) {
    size_t size = next_pow2(a.n + b.n - 1);
    return ifft(mul(fft(a, size), fft(b, size)), size).view(0, a.n + b.n - 1);
  }
  std::pair<DVec, DVec> fold(DVec v, size_t n) {       // divide_by_vanishing_poly -> (q, rem)
    DVec q = alloc(v.n > n ? v.n - n : 0), rem = alloc(n);
    poly_vanishing_fold(ctx, curve, v.p, v.n, n, q.n ? q.p : nullptr, rem.p);
    return {q, rem};
  }
  DVec spmv(const uint32_t* rp, const uint32_t* col, const uint64_t* cf, DVec x, size_t nrows) {
    DVec out = alloc(nrows);
    fr_spmv(ctx, curve, rp, col, cf, nrows, x.p, out.p);
    return out;
  }
  DVec gather(DVec v, const int32_t* idx_dev, size_t n) {
    DVec out = alloc(n);
    fr_gather(ctx, v.p, idx_dev, n, out.p);
    return out;
  }
  FrE element(DVec v, size_t i) {
    FrE e{};
    ZKP_HIP(hipMemcpyAsync(e.data(), v.p + 4 * i, 32, hipMemcpyDeviceToHost, st()));
    ZKP_HIP(hipStreamSynchronize(st()));
    return e;
  }
  FrE evaluate(DVec v, const FrE& z) {
    FrE out{};
    if (v.n == 0) return out;
    poly_div_linear(ctx, curve, v.p, v.n, reinterpret_cast<const uint64_t*>(z.data()), nullptr,
                    reinterpret_cast<uint64_t*>(out.data()));
    return out;
  }
};

struct DevCsr3 {
  uint32_t *rp = nullptr, *col = nullptr;
  uint64_t* cf = nullptr;
};

}  // namespace
}  // namespace zkp

using namespace zkp;

// ------------------------------------------------------------------------------------------------ index
struct zkp_marlin_index {
  int curve = 0;
  size_t ni = 0, n = 0, pad_aux = 0, nnz = 0, xs = 0, hs = 0, ks = 0, bs = 0, max_degree = 0;
  DevCsr3 csr[3], csr_t[3];
  DVec h_el;
  DVec on_k[3][3];     // row, col, val
  DVec on_b[3][4];     // row, col, val, row_col
  DVec polys[3][4];    // a_row, a_col, a_val, a_row_col, b_..., c_...  (Index::iter order, indexer.rs:51-67)
  int32_t *w_idx = nullptr, *x_idx = nullptr;
  std::vector<void*> owned;
  Pool pool;           // scratch of the provers that use this index
  uint64_t* early_pinned = nullptr;     // pinned landing zone of the early MSMs (EarlyMsms)
  ~zkp_marlin_index() {
    pool.trim();
    for (void* p : owned) (void)hipFree(p);
    if (early_pinned) (void)hipHostFree(early_pinned);
  }
};

namespace zkp {
namespace {

template <class T>
T* dev_copy(zkp_marlin_index* ix, hipStream_t st, const T* host, size_t count) {
  T* d = nullptr;
  if (hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
  ix->owned.push_back(d);
  if (count) ZKP_HIP(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st));
  return d;
}
DVec keep(zkp_marlin_index* ix, hipStream_t st, DVec v) {                // pool vector -> index-owned copy
  uint64_t* d = nullptr;
  if (hipMalloc(&d, std::max<size_t>(v.n, 1) * 32) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
  ix->owned.push_back(d);
  if (v.n) ZKP_HIP(hipMemcpyAsync(d, v.p, v.n * 32, hipMemcpyDeviceToDevice, st));
  return DVec{d, v.n};
}
size_t reindex_by_subdomain(size_t hs, size_t xs, size_t j) {             // ahp/constraint_systems.rs reindex_by_subdomain
  const size_t period = hs / xs;
  if (j < xs) return j * period;
  const size_t i = j - xs;
  return i + i / (period - 1) + 1;
}

}  // namespace

zkp_marlin_index* marlin_index_upload(zkp_ctx* ctx, const zkp_marlin_index_desc* d) {
  fr_require_curve(d->curve);
  ZKP_REQUIRE(d->num_inputs >= 1 && d->n >= d->num_inputs, ZKP_ERR_BAD_ARG);
  std::unique_ptr<zkp_marlin_index> ix(new zkp_marlin_index());
  ix->curve = d->curve;
  ix->ni = d->num_inputs;
  ix->n = d->n;
  ix->pad_aux = d->pad_aux;
  const zkp_csr* M[3] = {&d->a, &d->b, &d->c};
  size_t nnz = 0;
  for (auto* m : M) {
    ZKP_REQUIRE(m->row_ptr != nullptr, ZKP_ERR_BAD_ARG);
    nnz = std::max<size_t>(nnz, m->row_ptr[d->n]);
  }
  ZKP_REQUIRE(nnz >= 1, ZKP_ERR_BAD_ARG);
  ix->nnz = nnz;
  const size_t xs = next_pow2(ix->ni), hs = next_pow2(ix->n), ks = next_pow2(nnz), bs = next_pow2(3 * ks - 3);
  const int two_adicity = d->curve == ZKP_BN254 ? 28 : 32;
  ZKP_REQUIRE(log2_ceil(bs) + 1 <= two_adicity && hs > xs, ZKP_ERR_DOMAIN_TOO_LARGE);
  ix->xs = xs;
  ix->hs = hs;
  ix->ks = ks;
  ix->bs = bs;
  ix->max_degree = std::max(3 * hs + 2 * 1 - 1, 3 * ks - 3);              // ahp/mod.rs:66-84, zk_bound = 1
  Backend be{ctx, d->curve, fr_field(d->curve), &ix->pool};
  hipStream_t st = be.st();
  // H as a device vector: the evaluations of X over the domain
  DVec xpoly = be.zeros(hs);
  be.add_at(xpoly, 1, be.F.one_());
  ix->h_el = keep(ix.get(), st, be.fft(xpoly, hs));
  const DVec h_el = ix->h_el;
  for (int m = 0; m < 3; m++) {
    DVec diag_inv = be.scale(h_el, be.F.inverse(be.F.from_u64(hs)));   // diagonal_evals^-1 = u / |H|; a pool vector: one per matrix
    const uint32_t* rp = M[m]->row_ptr;
    const size_t k = rp[d->n];
    ix->csr[m].rp = dev_copy(ix.get(), st, rp, d->n + 1);
    ix->csr[m].col = dev_copy(ix.get(), st, M[m]->col, k);
    ix->csr[m].cf = dev_copy(ix.get(), st, M[m]->coeff, k * 4);
    // transposed, re-indexed matrix: t_on_h[kk] = sum_{(i, j): reindex(j) = kk} coeff * r_alpha[i]   (prover.rs:259-269)
    std::vector<uint32_t> jj(k), rows(k), tptr(hs + 1, 0), tcol(k);
    std::vector<uint64_t> tcf(k * 4 + 4);
    for (size_t i = 0; i < d->n; i++)
      for (uint32_t e = rp[i]; e < rp[i + 1]; e++) {
        rows[e] = (uint32_t)i;
        ZKP_REQUIRE(M[m]->col[e] < d->n, ZKP_ERR_BAD_ARG);
        jj[e] = (uint32_t)reindex_by_subdomain(hs, xs, M[m]->col[e]);
        tptr[jj[e] + 1]++;
      }
    for (size_t i = 0; i < hs; i++) tptr[i + 1] += tptr[i];
    {
      std::vector<uint32_t> cur(tptr.begin(), tptr.end() - 1);
      for (size_t e = 0; e < k; e++) {                                      // stable: entry order within a target row kept
        const uint32_t pos = cur[jj[e]]++;
        tcol[pos] = rows[e];
        memcpy(&tcf[4 * (size_t)pos], M[m]->coeff + 4 * e, 32);
      }
    }
    ix->csr_t[m].rp = dev_copy(ix.get(), st, tptr.data(), hs + 1);
    ix->csr_t[m].col = dev_copy(ix.get(), st, tcol.data(), k);
    ix->csr_t[m].cf = dev_copy(ix.get(), st, tcf.data(), k * 4);
    // row / col / val over K (arithmetic.rs:98-172), padded to |K| with (h_0, h_0, 0)
    std::vector<int32_t> irow(ks, 0), icol(ks, 0), idiag(ks, -1);
    std::vector<uint64_t> vcf(ks * 4, 0);
    for (size_t e = 0; e < k; e++) {
      irow[e] = (int32_t)jj[e];
      icol[e] = (int32_t)rows[e];
      idiag[e] = (int32_t)jj[e];
    }
    memcpy(vcf.data(), M[m]->coeff, k * 32);
    int32_t* d_irow = dev_copy(ix.get(), st, irow.data(), ks);
    int32_t* d_icol = dev_copy(ix.get(), st, icol.data(), ks);
    int32_t* d_idiag = dev_copy(ix.get(), st, idiag.data(), ks);
    DVec row = be.gather(h_el, d_irow, ks), colv = be.gather(h_el, d_icol, ks);
    DVec val = be.mul(be.upload(vcf.data(), ks), be.gather(diag_inv, d_idiag, ks));
    DVec rc = be.mul(row, colv);
    ZKP_HIP(hipStreamSynchronize(st));                 // the host staging vectors of this matrix die here
    DVec ev[4] = {row, colv, val, rc};
    for (int q = 0; q < 3; q++) ix->on_k[m][q] = keep(ix.get(), st, ev[q]);
    for (int q = 0; q < 4; q++) {
      DVec p = be.ifft(ev[q], ks);
      ix->polys[m][q] = keep(ix.get(), st, p);
      ix->on_b[m][q] = keep(ix.get(), st, be.fft(p, bs));
    }
    ix->pool.release_all();
  }
  // w_evals_on_h[i] = 0 if i % ratio == 0 else w_ext[i - i/ratio - 1] - x_evals_on_h[i]   (prover.rs:176-186)
  {
    const size_t ratio = hs / xs;
    std::vector<int32_t> wi(hs), xi(hs);
    for (size_t i = 0; i < hs; i++) {
      const bool in_x = i % ratio == 0;
      wi[i] = in_x ? -1 : (int32_t)(i - i / ratio - 1);
      xi[i] = in_x ? -1 : (int32_t)i;
    }
    ix->w_idx = dev_copy(ix.get(), st, wi.data(), hs);
    ix->x_idx = dev_copy(ix.get(), st, xi.data(), hs);
    ZKP_HIP(hipStreamSynchronize(st));
  }
  ix->pool.trim();
  return ix.release();
}

void marlin_index_info(const zkp_marlin_index* ix, uint64_t info[6]) {
  const uint64_t v[6] = {ix->xs, ix->hs, ix->ks, ix->bs, ix->max_degree, ix->nnz};
  memcpy(info, v, sizeof v);
}

void marlin_index_free(zkp_ctx* ctx, zkp_marlin_index* ix) {
  ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));
  delete ix;
}

// -> index_commitments[12] (affine Montgomery + identity flags), Index::iter order (lib.rs:77-83)
void marlin_index_commit(zkp_ctx* ctx, zkp_marlin_index* ix, uint64_t powers_g, uint64_t* comms_xy, uint8_t* inf) {
  const MsmVtbl* v1 = msm_vtbl(ix->curve, 1);
  const size_t jw64 = 3 * (size_t)v1->fN / 2;
  for (int m = 0; m < 3; m++)
    for (int q = 0; q < 4; q++) {
      std::vector<uint64_t> jac(jw64);
      MsmJob job;
      job.handle = powers_g;
      job.scalars_dev = ix->polys[m][q].p;
      job.n = ix->polys[m][q].n;
      job.montgomery = true;
      job.out_xyz_host = jac.data();
      msm_run(ctx, job);
      point_into_affine(ctx, ix->curve, 1, jac.data(), comms_xy + (size_t)(4 * m + q) * 12, inf + 4 * m + q);
    }
}

// ------------------------------------------------------------------------------------------------ prover
namespace {

// the canonical bytes (4 * F.N of them) of one element of F, Montgomery in: how ark writes a field element
void put_canonical(std::vector<uint8_t>& out, const HostField& F, const void* mont) {
  FrE a{};
  memcpy(a.data(), mont, 4 * F.N);
  const FrE c = F.to_canonical(a);
  const uint8_t* b = reinterpret_cast<const uint8_t*>(c.data());
  out.insert(out.end(), b, b + 4 * F.N);
}
// Fr elements as the host argument array of a fused kernel: 4 words each
void pack_fr(uint64_t* kh, std::initializer_list<FrE> els) {
  for (const FrE& e : els) {
    memcpy(kh, e.data(), 32);
    kh += 4;
  }
}

struct Challenger {                                    // lib.rs:105-158
  zkp_fs_rng* rng = nullptr;
  const uint64_t* fixed = nullptr;                     // 7 x 4 limbs Montgomery: alpha, eta_a, eta_b, eta_c, beta, gamma, xi
  int curve;
  HostField Fr, Fq;
  int log_hs;
  ~Challenger() {
    if (rng) zkp_fs_rng_free(rng);
  }
  // GroupAffine::write: x, y, infinity byte; ark's zero() is (0, 1, true)
  void put_g1(std::vector<uint8_t>& out, const uint64_t* xy, bool inf) const {
    if (inf) {
      out.insert(out.end(), 4 * Fq.N, 0);
      std::vector<uint8_t> one(4 * Fq.N, 0);
      one[0] = 1;
      out.insert(out.end(), one.begin(), one.end());
      out.push_back(1);
      return;
    }
    put_canonical(out, Fq, xy);
    put_canonical(out, Fq, reinterpret_cast<const uint32_t*>(xy) + Fq.N);
    out.push_back(0);
  }
  void absorb(const std::vector<uint8_t>& b) {
    if (rng) zkp_fs_rng_absorb(rng, b.data(), b.size());
  }
  // verifier message i of `fixed`, or the transcript's next one: a field element, or one outside H (ahp/verifier.rs:53-56,76)
  FrE next(int i, bool outside_h = false) {
    if (!rng) return fr_host_load(fixed + 4 * i);
    FrE e{};
    if (outside_h) zkp_fs_rng_sample_outside_domain(rng, (zkp_curve_t)curve, (uint32_t)log_hs, reinterpret_cast<uint64_t*>(e.data()));
    else zkp_fs_rng_rand_fr(rng, (zkp_curve_t)curve, reinterpret_cast<uint64_t*>(e.data()));
    return e;
  }
};

struct Commitment {
  std::vector<uint64_t> xy, sxy;                       // affine Montgomery; sxy empty = no degree bound
  uint8_t inf = 0, sinf = 0;
};

// label order used everywhere below: first round w, z_a, z_b, mask; second t, g_1, h_1; third g_2, h_2
enum { W_, ZA_, ZB_, MASK_, T_, G1_, H1_, G2_, H2_, NLAB };
struct Label {
  const char* name;
  bool bounded, hide;                                  // committed with a degree bound (a second, shifted commitment) / with a blinder
};
constexpr Label LABELS[NLAB] = {{"w", false, true},   {"z_a", false, true},  {"z_b", false, true},  {"mask", false, false}, {"t", false, false},
                                {"g_1", true, true},  {"h_1", false, false}, {"g_2", true, false},  {"h_2", false, false}};
size_t degree_bound(const zkp_marlin_index* ix, int l) { return l == G1_ ? ix->hs - 2 : l == G2_ ? ix->ks - 2 : 0; }

// Early commitments (round 3): a polynomial that is final long before its round ends (the mask polynomial — an input — and t(X)
// of the second round) starts its commitment MSM at once on an MSM workspace stream of this lane, under the NTTs / pointwise
// kernels that compute the rest of the round (which otherwise run alone: 12.6 + 4.9 ms per proof in a kernel trace);
// commit_round collects the result instead of launching the MSM.  ZKP_MARLIN_EARLY=0: every MSM inside commit_round.
struct EarlyMsms {
  static constexpr int MAX = 16;                       // pinned slots of an index
  static constexpr size_t SLOT = 24;                   // u64 words of a slot: a Jacobian G1 point of either curve (at most 18)
  struct Early {
    int label, ws;
    bool shifted;
    int kind;               // 0: commitment MSM over powers_of_g; 1: blinding MSM over powers_of_gamma_g (label / shifted: whose);
  };                        // 2: blinding term of opening proof `label`
  zkp_ctx* ctx;
  zkp_marlin_index* ix;
  uint64_t powers_g, powers_gamma_g;
  size_t jw64;
  std::vector<Early> list;
  EarlyMsms(zkp_ctx* c, zkp_marlin_index* i, uint64_t g, uint64_t gamma_g, size_t jw) : ctx(c), ix(i), powers_g(g), powers_gamma_g(gamma_g), jw64(jw) {
    if (!ix->early_pinned) ZKP_HIP(hipHostMalloc(reinterpret_cast<void**>(&ix->early_pinned), MAX * SLOT * 8));
  }
  // -> index into `list` (-1: not started, the caller runs the MSM itself later).  offset: first SRS power (shifted commitments)
  int start(int label, const DVec& v, size_t offset = 0, bool shifted = false, int kind = 0) {
    if (!ctx->tune.marlin_early || (int)list.size() >= MAX || v.n == 0) return -1;
    zkp_lane* L = ctx->cur;
    const int w = 1 + (int)(list.size() % (zkp_lane::N_WS_MSM - 1));
    hipStream_t ws_st = L->ws[w].stream;
    const uint64_t handle = kind == 0 ? powers_g : powers_gamma_g;
    ZKP_HIP(hipEventRecord(L->ev_fork, L->stream));                  // v is complete on the prover's stream
    ZKP_HIP(hipStreamWaitEvent(ws_st, L->ev_fork, 0));
    ZKP_REQUIRE(offset <= bases_len(ctx, handle), ZKP_ERR_BAD_ARG);
    MsmJob job;
    job.handle = handle;
    job.offset = offset;
    job.scalars_dev = v.p;
    job.n = std::min(v.n, bases_len(ctx, handle) - offset);             // ark min(len) truncation, as msm_run_multi
    job.montgomery = true;
    job.ws = w;
    msm_run(ctx, job);
    ZKP_HIP(hipMemcpyAsync(ix->early_pinned + list.size() * SLOT, L->ws[w].out.p, jw64 * 8, hipMemcpyDeviceToHost, ws_st));
    ZKP_HIP(hipEventRecord(L->ws[w].done, ws_st));
    list.push_back({label, w, shifted, kind});
    return (int)list.size() - 1;
  }
  int find(int label, bool shifted, int kind) const {
    for (size_t e = 0; e < list.size(); e++)
      if (list[e].label == label && list[e].shifted == shifted && list[e].kind == kind) return (int)e;
    return -1;
  }
  // (early MSM, destination of its Jacobian result: jw64 words) pairs: the prover's stream waits for every workspace stream
  // involved, the host for the prover's stream ONCE, then the pinned slots are read
  void collect(const std::vector<std::pair<int, uint64_t*>>& want) {
    if (want.empty()) return;
    for (auto& w : want) ZKP_HIP(hipStreamWaitEvent(ctx->cur->stream, ctx->cur->ws[list[w.first].ws].done, 0));
    ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));
    for (auto& w : want) memcpy(w.second, ix->early_pinned + (size_t)w.first * SLOT, jw64 * 8);
  }
};

// one MSM of a batch over one base vector: already running early (index into EarlyMsms::list) or -1
struct MsmItem {
  int early;
  const uint64_t* scalars;
  size_t n, offset;                                    // offset: first SRS power
};

struct Q {                                             // one entry of the query set
  std::string label;
  DVec p;
  bool at_beta;
  int l;                                               // prover label index or -1 (index polynomial)
};

// Pool memory and the index's pinned slots are recycled by the next proof: on EVERY exit (an exception between an early
// commitment and the round that collects it included) the prover's stream and the lane's MSM workspace streams are drained
// before the pool lets go of anything an in-flight MSM or its read-back may still touch.
struct Release {
  Pool* p;
  zkp_lane* lane;
  hipStream_t st;
  ~Release() {
    for (int w = 1; w < zkp_lane::N_WS; w++)
      if (lane->ws[w].stream) (void)hipStreamSynchronize(lane->ws[w].stream);
    (void)hipStreamSynchronize(st);
    p->release_all();
  }
};


// One proof: lib.rs:97-181 phase by phase.  run() is the sequence; what one phase leaves for a later one is a member.
struct Prover {
  using Clock = std::chrono::steady_clock;
  zkp_ctx* const ctx;
  zkp_marlin_index* const ix;
  const uint64_t powers_g, powers_gamma_g;
  const uint64_t *const x_mont, *const w_mont;
  const size_t n_w;
  const zkp_marlin_rand* const rnd;
  zkp_marlin_proof* const out;
  const int curve;
  Backend be;
  const HostField& F;
  const size_t aw64, jw64;                             // u64 words of an affine / Jacobian G1 point
  const size_t xs, hs, ks, bs, D, ni;
  const hipStream_t st;
  Challenger chal;
  EarlyMsms early;
  zkp_marlin_timing tm{};
  Clock::time_point t_begin, t_mark;
  DVec poly[NLAB];
  Commitment comm[NLAB];
  const uint64_t* blind_host[NLAB];                    // the hiding blinders (inputs), two coefficients each; g_1's shifted one apart
  DVec blind_dev[NLAB], blind_s_dev;
  DVec x_poly, z_poly, ZA_early, ZB_early, ZZ_early;   // first round -> second round
  size_t r2_size = 0;
  FrE alpha, etas[3], beta, gamma, xi, v_alpha;        // the verifier's messages; v_H(alpha)
  uint64_t beta_evals[4 * G2_];                        // ZKP_MARLIN_EARLY_EVAL: third round -> evaluations
  std::vector<Q> query;
  // LAST member, so destroyed FIRST: the streams are drained and the pool emptied before the early-MSM queue, the device vectors
  // above and everything else that in-flight work may touch goes away — on every exit from run(), exceptions included
  Release release;

  Prover(zkp_ctx* c, zkp_marlin_index* i, uint64_t g, uint64_t gamma_g, const uint8_t* ivk_bytes, size_t ivk_len, const uint64_t* x,
         const uint64_t* w, size_t nw, const zkp_marlin_rand* r, const uint64_t* fixed_challenges, zkp_marlin_proof* o)
      : ctx(c), ix(i), powers_g(g), powers_gamma_g(gamma_g), x_mont(x), w_mont(w), n_w(nw), rnd(r), out(o), curve(i->curve),
        be{c, i->curve, fr_field(i->curve), &i->pool}, F(be.F), aw64((size_t)msm_vtbl(i->curve, 1)->fN),
        jw64(3 * (size_t)msm_vtbl(i->curve, 1)->fN / 2), xs(i->xs), hs(i->hs), ks(i->ks), bs(i->bs), D(i->max_degree), ni(i->ni),
        st(be.st()), early(c, i, g, gamma_g, jw64),
        blind_host{r->blind_w, r->blind_z_a, r->blind_z_b, nullptr, nullptr, r->blind_g_1, nullptr, nullptr, nullptr},
        release{&i->pool, c->cur, st} {
    t_begin = t_mark = Clock::now();
    chal.curve = curve;
    chal.Fr = F;
    chal.Fq = fq_field(curve);
    chal.log_hs = log2_ceil(hs);
    chal.fixed = fixed_challenges;
    if (!fixed_challenges) {
      // FiatShamirRng::from_seed(&to_bytes![index_verifier_key, public_input])  (lib.rs:105-106); public input = x[1..]
      ZKP_REQUIRE(ivk_bytes != nullptr, ZKP_ERR_BAD_ARG);
      std::vector<uint8_t> seed(ivk_bytes, ivk_bytes + ivk_len);
      for (size_t k = 1; k < ni; k++) put_canonical(seed, F, x_mont + 4 * k);
      ZKP_REQUIRE(zkp_fs_rng_new(seed.data(), seed.size(), &chal.rng) == ZKP_OK, ZKP_ERR_OOM);
    }
  }

  void lap(double* dst) {                              // phase boundary: the stream is drained, the host clock read
    ZKP_HIP(hipStreamSynchronize(st));
    auto now = Clock::now();
    *dst += std::chrono::duration<double, std::milli>(now - t_mark).count();
    t_mark = now;
  }
  // a polynomial that is final: its commitment MSM (and the one against the shifted powers of a degree-bounded polynomial) starts now
  void commit_early(int l) {
    (void)early.start(l, poly[l]);
    if (LABELS[l].bounded) (void)early.start(l, poly[l], D - degree_bound(ix, l), true);
  }

  // A batch of MSMs over one base vector -> jac[i * jw64 ...] in item order.  ONE batched call for the items that are not running
  // early; the early ones are waited for after it is launched.
  void run_msms(uint64_t handle, const std::vector<MsmItem>& items, uint64_t* jac) {
    std::vector<size_t> offs, ns, at;
    std::vector<const uint64_t*> ptrs;
    std::vector<std::pair<int, uint64_t*>> running;
    for (size_t i = 0; i < items.size(); i++) {
      if (items[i].early >= 0) {
        running.push_back({items[i].early, jac + i * jw64});
        continue;
      }
      at.push_back(i);
      offs.push_back(items[i].offset);
      ns.push_back(items[i].n);
      ptrs.push_back(items[i].scalars);
    }
    std::vector<uint64_t> part(std::max<size_t>(ptrs.size(), 1) * jw64);
    msm_run_batch(ctx, handle, ptrs.size(), offs.data(), ptrs.data(), ns.data(), true, part.data());
    early.collect(running);
    for (size_t k = 0; k < at.size(); k++) memcpy(jac + at[k] * jw64, part.data() + k * jw64, jw64 * 8);
  }

  // PC::commit (pc/mod.rs:34-71) of one round: one batched MSM call per base vector
  void commit_round(std::initializer_list<int> labels) {
    std::vector<std::pair<int, bool>> slot;                          // (label, shifted) of every commitment of the round
    std::vector<MsmItem> items, bitems;
    std::vector<size_t> bslot;                                       // the slot a blinding MSM belongs to
    for (int l : labels)
      for (int sh = 0; sh <= (LABELS[l].bounded ? 1 : 0); sh++) {
        slot.push_back({l, sh != 0});
        // shifted_powers(bound) = powers[D - bound ..]
        items.push_back({early.find(l, sh != 0, 0), poly[l].p, poly[l].n, sh ? D - degree_bound(ix, l) : 0});
        tm.commit_points += poly[l].n;
        if (!LABELS[l].hide) continue;
        bslot.push_back(slot.size() - 1);
        bitems.push_back({early.find(l, sh != 0, 1), sh ? blind_s_dev.p : blind_dev[l].p, 2, 0});
      }
    std::vector<uint64_t> jac(slot.size() * jw64), bjac(std::max<size_t>(bitems.size(), 1) * jw64);
    run_msms(powers_g, items, jac.data());
    run_msms(powers_gamma_g, bitems, bjac.data());
    // commitment k = affine(MSM_k + blinding MSM_k): all of the round in ONE launch (a single-lane inversion each, side by side)
    std::vector<uint64_t> bj(slot.size() * jw64, 0), axy(slot.size() * aw64);
    std::vector<uint8_t> has(slot.size(), 0), ainf(slot.size(), 0);
    for (size_t b = 0; b < bslot.size(); b++) {
      has[bslot[b]] = 1;
      memcpy(bj.data() + bslot[b] * jw64, bjac.data() + b * jw64, jw64 * 8);
    }
    if (ctx->tune.marlin_host_affine) {
      std::vector<HostJac> pts(slot.size());
      for (size_t k = 0; k < slot.size(); k++) {
        pts[k] = host_jac_load(chal.Fq, jac.data() + k * jw64);
        if (has[k]) pts[k] = host_jac_add(chal.Fq, pts[k], host_jac_load(chal.Fq, bj.data() + k * jw64));
      }
      host_into_affine(chal.Fq, pts, axy.data(), aw64, ainf.data());
    } else {
      points_fold_into_affine(ctx, curve, 1, jac.data(), bj.data(), has.data(), slot.size(), axy.data(), ainf.data());
    }
    for (size_t k = 0; k < slot.size(); k++) {
      Commitment& c = comm[slot[k].first];
      std::vector<uint64_t>& dst = slot[k].second ? c.sxy : c.xy;
      dst.assign(axy.begin() + k * aw64, axy.begin() + (k + 1) * aw64);
      (slot[k].second ? c.sinf : c.inf) = ainf[k];
    }
    // to_bytes![round commitments]: comm, shifted_exists byte, shifted or the empty commitment (pc/data_structures.rs:143-154)
    std::vector<uint8_t> bytes;
    for (int l : labels) {
      chal.put_g1(bytes, comm[l].xy.data(), comm[l].inf != 0);
      bytes.push_back(LABELS[l].bounded ? 1 : 0);
      if (LABELS[l].bounded) chal.put_g1(bytes, comm[l].sxy.data(), comm[l].sinf != 0);
      else chal.put_g1(bytes, nullptr, true);
    }
    chal.absorb(bytes);
  }

  // the mask polynomial is an input: prepared first so that its commitment (the largest MSM of the round) runs under the
  // interpolations of the first round
  void prepare_mask_and_blinders() {
    const size_t mask_len = 3 * hs + 2 * 1 - 2;
    DVec mask = be.alloc(mask_len);
    ZKP_HIP(hipMemcpyAsync(mask.p, rnd->mask, mask_len * 32, rnd->mask_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    DVec mrem = be.fold(mask, hs).second;
    be.add_at(mask, 0, F.neg(be.element(mrem, 0)));     // mask - sigma_H(mask)/|H| ... exactly prover.rs:202-205
    poly[MASK_] = mask;
    commit_early(MASK_);
    // the hiding blinders are inputs too: their two-term MSMs over powers_of_gamma_g (one full bucket pipeline each: ~1 ms of latency-
    // bound launches, little work) start now and are collected by the round that needs them — they used to run as a second, blocking
    // batch behind the commitment MSMs of every round
    for (int l = 0; l < NLAB; l++)
      if (LABELS[l].hide) blind_dev[l] = be.upload(blind_host[l], 2);
    blind_s_dev = be.upload(rnd->blind_shifted_g_1, 2);
    for (int l = 0; l < NLAB; l++)
      if (LABELS[l].hide) {
        (void)early.start(l, blind_dev[l], 0, false, 1);
        if (LABELS[l].bounded) (void)early.start(l, blind_s_dev, 0, true, 1);
      }
  }

  // prover_init (prover.rs:86-147) and the first round (prover.rs:150-222)
  void first_round() {
    // (round 4: the witness crosses PCIe from pageable host memory AFTER the mask MSM is under way — the copy blocks the host for
    //  about a millisecond, during which the device used to idle)
    // ---- prover_init: z = x ++ w ++ padding ones; z_a = A z, z_b = B z
    DVec z = be.alloc(ix->n);
    ZKP_HIP(hipMemcpyAsync(z.p, x_mont, ni * 32, hipMemcpyHostToDevice, st));
    if (n_w) ZKP_HIP(hipMemcpyAsync(z.p + 4 * ni, w_mont, n_w * 32, hipMemcpyHostToDevice, st));
    if (ix->pad_aux) {
      DVec ones = be.zeros(ix->pad_aux);
      DVec tgt = z.view(ni + n_w, ix->n);
      const FrE o = F.one_();
      be.op(ZKP_VEC_ADDC, ones, nullptr, tgt, ix->pad_aux, &o);
    }
    DVec z_a_ev = be.spmv(ix->csr[0].rp, ix->csr[0].col, ix->csr[0].cf, z, ix->n);
    DVec z_b_ev = be.spmv(ix->csr[1].rp, ix->csr[1].col, ix->csr[1].cf, z, ix->n);
    // ---- first round
    x_poly = be.ifft(z.view(0, ni), xs);
    DVec x_on_h = be.fft(x_poly, hs);
    DVec w_ext = be.pad(z.view(ni), hs - xs);
    DVec w_on_h = be.sub(be.gather(w_ext, ix->w_idx, hs), be.gather(x_on_h, ix->x_idx, hs));
    auto masked = [this](DVec ev, const FrE& r) {       // interpolate(ev) + r * v_H
      DVec p = be.pad(be.ifft(ev, hs), hs + 1);
      be.add_at(p, 0, F.neg(r));
      be.add_at(p, hs, r);
      return p;
    };
    DVec w_poly = be.fold(masked(w_on_h, fr_host_load(rnd->w)), xs).first;
    poly[W_] = w_poly;
    commit_early(W_);                                    // under the interpolations of z_a and z_b
    poly[ZA_] = masked(z_a_ev, fr_host_load(rnd->z_a));
    commit_early(ZA_);
    poly[ZB_] = masked(z_b_ev, fr_host_load(rnd->z_b));
    // Round 5: three of the five product-domain transforms of the SECOND round (z_a, z_b and z = w v_X + x over the 4|H| domain) do not
    // depend on the verifier's first message, and the first round leaves the device under-used while its early commitment MSMs drain
    // (kernel trace: accumulate 0.4-0.9 of the time, nothing else): they run here instead of alone after alpha is known (3.5 ms of
    // transforms with no MSM to overlap).  MEASURED NEUTRAL (profiles/r05_marlin_ab.txt: rounds 1 + 2 incl.
    // commits 16.1 ms without, 16.5 with: the first round's early MSMs simply take the vector ALUs the transforms left, the device is
    // saturated either way), so it is OFF by default; ZKP_MARLIN_EARLY_FFT=1 enables it; same proof bytes.
    z_poly = be.axpy(be.sub(be.shift(w_poly, xs), w_poly), x_poly, F.one_());      // w * v_X + x  (prover.rs:277-281)
    // r_alpha and t have |H| coefficients
    r2_size = next_pow2(std::max({poly[MASK_].n, hs + (poly[ZA_].n + poly[ZB_].n - 1), hs + z_poly.n}));
    if (ctx->tune.marlin_early_fft) {
      ZA_early = be.fft(poly[ZA_], r2_size);
      ZB_early = be.fft(poly[ZB_], r2_size);
      ZZ_early = be.fft(z_poly, r2_size);
    }
  }

  // prover.rs:230-321
  void second_round() {
    const FrE one = F.one_();
    const DVec z_a = poly[ZA_], z_b = poly[ZB_], mask = poly[MASK_];
    v_alpha = F.sub(F.pow2k(alpha, log2_ceil(hs)), one);
    DVec r_alpha_on_h = be.scale(be.binv(be.addc(be.scale(ix->h_el, F.neg(one)), alpha)), v_alpha);
    DVec r_alpha = be.ifft(r_alpha_on_h, hs);
    DVec t_on_h = be.zeros(hs);
    for (int m = 0; m < 3; m++)
      be.axpy_into(t_on_h, be.spmv(ix->csr_t[m].rp, ix->csr_t[m].col, ix->csr_t[m].cf, r_alpha_on_h, hs), etas[m]);
    DVec t_poly = be.ifft(t_on_h, hs);
    poly[T_] = t_poly;
    commit_early(T_);                                                        // under the product FFTs below
    // m(X) = eta_c z_a z_b + eta_a z_a + eta_b z_b (z_a.n + z_b.n - 1 coefficients) is formed pointwise over the product domain
    const size_t m_n = z_a.n + z_b.n - 1;
    const size_t size = next_pow2(std::max({mask.n, r_alpha.n + m_n, t_poly.n + z_poly.n}));
    DVec prod = be.alloc(size);
    {
      const bool pre = ctx->tune.marlin_early_fft && size == r2_size;
      DVec RA = be.fft(r_alpha, size), TT = be.fft(t_poly, size);
      DVec ZA = pre ? ZA_early : be.fft(z_a, size), ZB = pre ? ZB_early : be.fft(z_b, size), ZZ = pre ? ZZ_early : be.fft(z_poly, size);
      uint64_t kh[3 * 4];
      pack_fr(kh, {etas[0], etas[1], etas[2]});
      marlin_round2_prod(ctx, curve, RA.p, ZA.p, ZB.p, TT.p, ZZ.p, kh, prod.p, size);
    }
    DVec q1 = be.axpy(be.ifft(prod, size), mask, one);
    auto hx = be.fold(q1, hs);
    poly[G1_] = hx.second.view(1, hs);
    poly[H1_] = hx.first.view(0, 2 * hs);
  }

  // prover.rs:331-427
  void third_round() {
    const FrE v_beta = F.sub(F.pow2k(beta, log2_ceil(hs)), F.one_());
    const FrE vab = F.mul(v_alpha, v_beta);
    const FrE eta_vab[3] = {F.mul(etas[0], vab), F.mul(etas[1], vab), F.mul(etas[2], vab)};
    DVec acc = be.alloc(ks);                              // = v_H(alpha) v_H(beta) sum_m eta_m val_m / ((beta - row_m)(alpha - col_m)) over K
    {
      const uint64_t* onk[9];
      for (int m = 0; m < 3; m++)
        for (int q = 0; q < 3; q++) onk[3 * m + q] = ix->on_k[m][q].p;
      uint64_t kh[5 * 4];
      pack_fr(kh, {alpha, beta, eta_vab[0], eta_vab[1], eta_vab[2]});
      marlin_t3_evals(ctx, curve, onk, kh, acc.p, ks);
    }
    DVec t3 = be.ifft(acc, ks);
    poly[G2_] = t3.view(1, ks);
    commit_early(G2_);                                   // g_2 and its shifted commitment run under the |B|-sized transforms below
    const FrE ab = F.mul(alpha, beta);
    if (4 * ks - 3 <= bs && ks >= 4) {
      // (a - b t) over B in one fused pass + ONE inverse transform: b's evaluations over B are already the transform pmul would
      // recompute (|B| >= deg(b t) + 1: no wrap-around), so the interpolations of a and b and the forward transform of b_poly drop out
      // (five transforms of size |B| -> two); see marlin_h2_numerator (poly.hip)
      DVec t_on_b = be.fft(t3, bs);
      const uint64_t* onb[12];
      for (int m = 0; m < 3; m++)
        for (int q = 0; q < 4; q++) onb[4 * m + q] = ix->on_b[m][q].p;
      uint64_t kh[6 * 4];
      pack_fr(kh, {alpha, beta, ab, eta_vab[0], eta_vab[1], eta_vab[2]});
      DVec num = be.alloc(bs);
      marlin_h2_numerator(ctx, curve, onb, t_on_b.p, kh, num.p, bs);
      DVec h2 = be.fold(be.ifft(num, bs).view(0, 4 * ks - 3), ks).first;
      poly[H2_] = h2.view(0, 3 * ks - 3);
    } else {
      DVec den[3];
      for (int m = 0; m < 3; m++)
        den[m] = be.addc(be.axpy(be.axpy(ix->on_b[m][3], ix->on_b[m][0], F.neg(alpha)), ix->on_b[m][1], F.neg(beta)), ab);
      DVec a_on_b = be.zeros(bs);
      for (int m = 0; m < 3; m++)
        be.axpy_into(a_on_b, be.mul(be.mul(ix->on_b[m][2], den[(m + 1) % 3]), den[(m + 2) % 3]), etas[m]);
      DVec a_poly = be.ifft(be.scale(a_on_b, vab), bs);
      DVec b_poly = be.ifft(be.mul(be.mul(den[0], den[1]), den[2]), bs);
      DVec h2 = be.fold(be.sub(a_poly.view(0, 3 * ks - 2), be.pmul(b_poly.view(0, 3 * ks - 2), t3)), ks).first;
      poly[H2_] = h2.view(0, 3 * ks - 3);
    }
    // Round 5: h_2's commitment starts before the round's host synchronisation, and the seven evaluations at beta (first- and
    // second-round polynomials: all known since the second round) run under its bucket sort instead of after gamma is known
    // — MEASURED SLOWER (profiles/r05_marlin_ab.txt: evaluations 1.0 -> 0.8 ms, batch_open +0.7 ms): OFF by default, ZKP_MARLIN_EARLY_EVAL=1 enables
    if (ctx->tune.marlin_early_eval) {
      commit_early(H2_);
      const uint64_t* qp[G2_];
      size_t qn[G2_];
      uint64_t qz[4 * G2_];
      for (int l = 0; l < G2_; l++) {
        qp[l] = poly[l].p;
        qn[l] = poly[l].n;
        memcpy(qz + 4 * l, beta.data(), 32);
      }
      poly_evaluate_batch(ctx, curve, G2_, qp, qn, qz, beta_evals);
    }
  }

  // evaluations in query-set order: BTreeSet<(label, point)>, i.e. by label (lib.rs:147-156)
  void evaluations() {
    for (int l = 0; l < NLAB; l++) query.push_back({LABELS[l].name, poly[l], l < G2_, l});
    static const char* MAT[3] = {"a", "b", "c"};
    static const char* KIND[4] = {"row", "col", "val", "row_col"};
    for (int m = 0; m < 3; m++)
      for (int q = 0; q < 4; q++) query.push_back({std::string(MAT[m]) + "_" + KIND[q], ix->polys[m][q], false, -1});
    std::sort(query.begin(), query.end(), [](const Q& a, const Q& b) { return a.label < b.label; });
    ZKP_REQUIRE(query.size() == ZKP_MARLIN_NUM_EVALS, ZKP_ERR_BAD_ARG);
    // all 21 Horner chains are enqueued, then ONE read-back (a host round trip per polynomial cost 2.5 ms of a proof)
    std::vector<const uint64_t*> qp;
    std::vector<size_t> qn, slot;
    std::vector<uint64_t> qz;
    for (size_t i = 0; i < query.size(); i++) {
      if (ctx->tune.marlin_early_eval && query[i].at_beta && query[i].l >= 0) {      // evaluated under the h_2 commitment
        memcpy(out->evaluations + 4 * i, beta_evals + 4 * query[i].l, 32);
        continue;
      }
      qp.push_back(query[i].p.p);
      qn.push_back(query[i].p.n);
      slot.push_back(i);
      const FrE& pt = query[i].at_beta ? beta : gamma;
      qz.insert(qz.end(), reinterpret_cast<const uint64_t*>(pt.data()), reinterpret_cast<const uint64_t*>(pt.data()) + 4);
    }
    std::vector<uint64_t> ev(4 * std::max<size_t>(qp.size(), 1));
    poly_evaluate_batch(ctx, curve, qp.size(), qp.data(), qn.data(), qz.data(), ev.data());
    for (size_t k = 0; k < slot.size(); k++) memcpy(out->evaluations + 4 * slot[k], ev.data() + 4 * k, 32);
    std::vector<uint8_t> ev_bytes;
    for (size_t i = 0; i < query.size(); i++) put_canonical(ev_bytes, F, out->evaluations + 4 * i);
    chal.absorb(ev_bytes);                                                   // lib.rs:157
  }

  void squeeze_xi() {                                                        // lib.rs:158: u128::rand(..).into()
    if (!chal.rng) {
      xi = chal.next(6);
      return;
    }
    uint64_t xi128[2] = {0, 0};
    zkp_fs_rng_rand_u128(chal.rng, xi128);
    uint32_t limbs[8] = {(uint32_t)xi128[0], (uint32_t)(xi128[0] >> 32), (uint32_t)xi128[1], (uint32_t)(xi128[1] >> 32), 0, 0, 0, 0};
    xi = F.from_canonical(limbs);
  }

  struct Opening {                                     // one query point of batch_open
    FrE point;
    bool at_beta, all;                                 // which queries it answers: those at beta / at gamma, or all (beta == gamma)
    std::array<FrE, 2> rb;                             // the blinding polynomial rb0 + rb1 X of the combination
    DVec rb1_dev, witness;
    int rb_early = -1, w_early = -1;
    bool takes(const Q& q) const { return all || q.at_beta == at_beta; }
    bool has_rand(const HostField& F) const { return !F.is_zero(rb[0]) || !F.is_zero(rb[1]); }
  };

  // the blinding polynomial rb0 + rb1 X of every opening is a combination of INPUTS (the hiding blinders) with powers of xi: known
  // now.  Its witness at any point is the constant rb1, so the one-term MSMs rb1 * gamma_g[0] start here, under the combinations,
  // divisions and witness MSMs that follow (they used to run as a blocking batch at the very end of the proof).
  void opening_blinder(Opening& o, int k) {
    const FrE xi2 = F.mul(xi, xi);
    o.rb = {F.zero(), F.zero()};
    FrE c = F.one_();
    for (const Q& q : query) {
      if (!o.takes(q)) continue;
      const int l = q.l;
      if (l >= 0 && LABELS[l].hide)
        for (int i = 0; i < 2; i++) o.rb[i] = F.add(o.rb[i], F.mul(c, fr_host_load(blind_host[l] + 4 * i)));
      if (l >= 0 && LABELS[l].bounded && LABELS[l].hide) {
        const FrE sc = F.mul(c, xi);
        for (int i = 0; i < 2; i++) o.rb[i] = F.add(o.rb[i], F.mul(sc, fr_host_load(rnd->blind_shifted_g_1 + 4 * i)));
      }
      c = F.mul(c, xi2);
    }
    if (o.has_rand(F)) {
      o.rb1_dev = be.upload(std::vector<FrE>{o.rb[1]});
      o.rb_early = early.start(k, o.rb1_dev, 0, false, 2);
    }
  }

  // the combination of the point's polynomials with powers of xi, divided by (X - point)
  void opening_witness(Opening& o, bool start_early) {
    const FrE xi2 = F.mul(xi, xi);
    DVec p = be.zeros(D + 1);
    FrE c = F.one_();
    for (const Q& q : query) {
      if (!o.takes(q)) continue;
      be.axpy_into(p, q.p, c);
      const int l = q.l;
      if (l >= 0 && LABELS[l].bounded) be.axpy_into(p, q.p, F.mul(c, xi), D - degree_bound(ix, l));
      c = F.mul(c, xi2);
    }
    o.witness = be.alloc(D);
    poly_div_linear(ctx, curve, p.p, D + 1, reinterpret_cast<const uint64_t*>(o.point.data()), o.witness.p, nullptr);
    if (start_early) o.w_early = early.start(-1, o.witness);         // under the next point's combination + division
  }

  // PC::batch_open (pc/mod.rs:73-160): per query point (ascending), labels ascending
  void batch_open() {
    const int order = F.cmp_canonical(beta, gamma);
    const int npts = order == 0 ? 1 : 2;
    std::vector<Opening> op(npts);
    for (int k = 0; k < npts; k++) {
      op[k].at_beta = k == 0 ? order <= 0 : order > 0;
      op[k].all = order == 0;
      op[k].point = op[k].at_beta ? beta : gamma;
    }
    for (int k = 0; k < npts; k++) opening_blinder(op[k], k);
    for (int k = 0; k < npts; k++) opening_witness(op[k], k + 1 < npts);
    std::vector<MsmItem> items, bitems;
    for (const Opening& o : op) {
      items.push_back({o.w_early, o.witness.p, D, 0});
      if (o.has_rand(F)) bitems.push_back({o.rb_early, o.rb1_dev.p, 1, 0});
    }
    std::vector<uint64_t> wjac(npts * jw64), bj(std::max<size_t>(bitems.size(), 1) * jw64);
    tm.open_points += (uint64_t)npts * D;
    run_msms(powers_g, items, wjac.data());
    // witness of the blinding polynomial rb0 + rb1 X at the point: quotient rb1 (degree 0), rand_v = rb(point) = rb0 + rb1 z — host
    // arithmetic; the one-term MSMs rb1 * gamma_g[0] of both points run as ONE batched call (early MSMs off / slots exhausted) or
    // were started early, the sums and the affine conversions of both opening proofs on the host with one inversion (was: per point
    // an upload, a division launch chain, an MSM, a fold launch and an into_affine launch, each with its own synchronisation)
    run_msms(powers_gamma_g, bitems, bj.data());
    out->num_opening_proofs = (uint32_t)npts;
    std::vector<HostJac> hp(npts);
    for (int k = 0, b = 0; k < npts; k++) {
      hp[k] = host_jac_load(chal.Fq, wjac.data() + (size_t)k * jw64);
      out->opening_has_rand[k] = 0;
      memset(out->opening_rand_v + 4 * k, 0, 32);
      if (!op[k].has_rand(F)) continue;
      const FrE ev = F.add(op[k].rb[0], F.mul(op[k].rb[1], op[k].point));
      out->opening_has_rand[k] = 1;
      memcpy(out->opening_rand_v + 4 * k, ev.data(), 32);
      hp[k] = host_jac_add(chal.Fq, hp[k], host_jac_load(chal.Fq, bj.data() + (size_t)(b++) * jw64));
    }
    uint8_t oinf[2] = {0, 0};
    memset(out->opening_w, 0, sizeof out->opening_w);
    host_into_affine(chal.Fq, hp, out->opening_w, 12, oinf);
    for (int k = 0; k < npts; k++) out->opening_w_inf[k] = oinf[k];
  }

  void write_results() {
    for (int l = 0; l < NLAB; l++) {
      memset(out->comm + l * 12, 0, 96);
      memcpy(out->comm + l * 12, comm[l].xy.data(), aw64 * 8);
      out->comm_inf[l] = comm[l].inf;
    }
    memset(out->shifted, 0, sizeof out->shifted);
    memcpy(out->shifted, comm[G1_].sxy.data(), aw64 * 8);
    memcpy(out->shifted + 12, comm[G2_].sxy.data(), aw64 * 8);
    out->shifted_inf[0] = comm[G1_].sinf;
    out->shifted_inf[1] = comm[G2_].sinf;
    pack_fr(out->challenges, {alpha, etas[0], etas[1], etas[2], beta, gamma, xi});
  }

  void run() {
    prepare_mask_and_blinders();
    first_round();
    lap(&tm.ms_round[0]);
    commit_round({W_, ZA_, ZB_, MASK_});                                     // lib.rs:109-112
    lap(&tm.ms_commit[0]);
    alpha = chal.next(0, true);                                              // ahp/verifier.rs:53-56
    for (int m = 0; m < 3; m++) etas[m] = chal.next(1 + m);
    second_round();
    lap(&tm.ms_round[1]);
    commit_round({T_, G1_, H1_});                                            // lib.rs:117-120
    lap(&tm.ms_commit[1]);
    beta = chal.next(4, true);                                               // ahp/verifier.rs:76
    third_round();
    lap(&tm.ms_round[2]);
    commit_round({G2_, H2_});                                                // lib.rs:124-127
    lap(&tm.ms_commit[2]);
    gamma = chal.next(5);                                                    // ahp/verifier.rs:86
    evaluations();
    lap(&tm.ms_evaluations);
    squeeze_xi();
    batch_open();
    write_results();
    lap(&tm.ms_open);
    tm.ms_total = std::chrono::duration<double, std::milli>(Clock::now() - t_begin).count();
    tm.ntt_count = be.ntt_count;
    tm.ntt_elements = be.ntt_elements;
    ctx->last_marlin_timing = tm;
  }
};

}  // namespace

void marlin_prove(zkp_ctx* ctx, zkp_marlin_index* ix, uint64_t powers_g, uint64_t powers_gamma_g, const uint8_t* ivk_bytes,
                  size_t ivk_len, const uint64_t* x_mont, const uint64_t* w_mont, size_t n_w, const zkp_marlin_rand* rnd,
                  const uint64_t* fixed_challenges, zkp_marlin_proof* out) {
  ZKP_REQUIRE(msm_vtbl(ix->curve, 1)->fN <= 12, ZKP_ERR_BAD_ARG);         // an affine G1 point fits the proof's 12-word fields
  ZKP_REQUIRE(ix->ni + n_w + ix->pad_aux == ix->n, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(bases_len(ctx, powers_g) >= ix->max_degree + 1 && bases_len(ctx, powers_gamma_g) >= 2, ZKP_ERR_BAD_ARG);
  Prover(ctx, ix, powers_g, powers_gamma_g, ivk_bytes, ivk_len, x_mont, w_mont, n_w, rnd, fixed_challenges, out).run();
}

}  // namespace zkp
