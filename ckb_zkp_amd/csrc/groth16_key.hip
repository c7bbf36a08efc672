// The Groth16 proving key on the device: everything that builds, describes or frees a zkp_groth16_pk (groth16_pk.hpp).  The upload
// is a KeyBuild, phase by phase: the circuit's matrices, the slices and window plan of the whole key, the five query tables (the H
// query in evaluation form and C folded into the L query unless the key is kept as given), then which sorts and passes the prover's
// MSMs share.  The provers that read the key are in groth16.hip and groth16_multi.hip.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "field_dev.hpp"
#include "fr_dev.hpp"              // with_fr: only ever reached with a curve the upload has validated, its throw is unreachable here
#include "groth16_fold_plan.hpp"
#include "groth16_pk.hpp"
#include "host_field.hpp"
#include "internal.hpp"
#include "msm_vtbl.hpp"

using namespace zkp;

namespace zkp {

// out[i] = canonical(mult * base^i), 8 words each: the scalar tables of the key transforms (lagrange_h)
template <class P>
__global__ __launch_bounds__(256) void pow_canon_kernel(uint32_t* __restrict__ out, const uint32_t* __restrict__ base,
                                                        const uint32_t* __restrict__ mult, uint32_t count) {
  using F = Fp<P>;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  (F::load(base).pow_u64(i) * F::load(mult)).from_mont().store(out + (size_t)i * 8);
}

// consts[0] = (g^N - 1)^-1
template <class P>
__global__ void qap_consts_kernel(uint32_t* consts, int log_n) {
  if (threadIdx.x || blockIdx.x) return;
  using F = Fp<P>;
  F g;
#pragma unroll
  for (int i = 0; i < 8; i++) g.v[i] = P::GEN[i];
  for (int i = 0; i < log_n; i++) g = g.sqr();
  (g - F::one()).inv().store(consts);
}

static DevCsr upload_csr(zkp_ctx* ctx, const zkp_csr& m, uint32_t rows) {
  DevCsr d;
  ZKP_REQUIRE(m.row_ptr != nullptr, ZKP_ERR_BAD_ARG);
  d.nnz = m.row_ptr[rows];
  ZKP_REQUIRE(d.nnz == 0 || (m.col && m.coeff), ZKP_ERR_BAD_ARG);
  if (hipMalloc(&d.row_ptr, ((size_t)rows + 1) * 4) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
  if (hipMalloc(&d.col, std::max<size_t>(d.nnz, 1) * 4) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
  if (hipMalloc(&d.coeff, std::max<size_t>(d.nnz, 1) * 32) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
  ZKP_HIP(hipMemcpyAsync(d.row_ptr, m.row_ptr, ((size_t)rows + 1) * 4, hipMemcpyHostToDevice, ctx->cur->stream));
  if (d.nnz) {
    ZKP_HIP(hipMemcpyAsync(d.col, m.col, d.nnz * 4, hipMemcpyHostToDevice, ctx->cur->stream));
    ZKP_HIP(hipMemcpyAsync(d.coeff, m.coeff, d.nnz * 32, hipMemcpyHostToDevice, ctx->cur->stream));
  }
  return d;
}

// contiguous, balanced index ranges: the first (n % world) ranks get one extra element
static void shard_bounds(size_t n, int rank, int world, size_t* lo, size_t* cnt) {
  if (world <= 0) {
    *lo = 0;
    *cnt = n;
    return;
  }
  const size_t base = n / (size_t)world, rem = n % (size_t)world, r = (size_t)rank;
  *lo = r * base + std::min(r, rem);
  *cnt = base + (r < rem ? 1 : 0);
}
// query ++ tail points (tail entry nullptr = identity)
// only elements [lo, lo + cnt) of the extended query are uploaded (the whole of it for an unsharded key)
// `lead` identity points are put in front of the query (the L query is stored index-aligned with z: lead = num_inputs);
// flags_out (optional) receives the identity flags of the uploaded slice
static uint64_t upload_ext(zkp_ctx* ctx, int curve, int group, const uint64_t* q, const uint8_t* inf, size_t n,
                           size_t limbs_per_point, const uint64_t* const tail[4], size_t lo, size_t cnt, size_t lead = 0,
                           std::vector<uint8_t>* flags_out = nullptr, int c_hint = 0, int cap_hint = 0, int lgk = -1) {
  std::vector<uint64_t> xy(std::max<size_t>(cnt, 1) * limbs_per_point, 0);
  std::vector<uint8_t> fl(std::max<size_t>(cnt, 1), 0);
  for (size_t j = 0; j < cnt; j++) {
    if (lo + j < lead) {
      fl[j] = 1;
      continue;
    }
    const size_t i = lo + j - lead;
    if (i < n) {
      memcpy(xy.data() + j * limbs_per_point, q + i * limbs_per_point, limbs_per_point * 8);
      fl[j] = inf ? inf[i] : 0;
    } else if (tail[i - n]) {
      memcpy(xy.data() + j * limbs_per_point, tail[i - n], limbs_per_point * 8);
    } else {
      fl[j] = 1;
    }
  }
  if (flags_out) *flags_out = fl;
  return bases_upload(ctx, curve, group, xy.data(), fl.data(), cnt, c_hint, cap_hint, lgk);
}

static void lagrange_h(zkp_ctx* ctx, int curve, const uint64_t* h_query, const uint8_t* h_inf, size_t h_used, int log_n,
                       std::vector<uint64_t>* xy_out, std::vector<uint8_t>* inf_out, int mode);

// The H query in evaluation form (round 4).  h = coset_ifft(v) (r1cs_to_qap.rs:169) is linear, h_i = g^-i / N sum_j w^-ij v_j, so
//     sum_i h_i H_i = sum_j v_j H'_j     with     H'_j = sum_i w^-ij (g^-i / N) H_i
// — a group-element transform of the key, done once at upload (N log N / 2 scalar multiplications on the device, 0.5 s at 2^20),
// after which the prover feeds the pointwise values v = (a b - c) / Z(g) on the coset straight to the H MSM: 18 instead of 21
// transform passes per proof and one transform less on the witness map -> H chain.  The proof is the same group element; terms
// beyond min(h_len, N) are the identity (prover.rs:186-187 truncates there).  ZKP_H_LAGRANGE=0: the coefficient-form key.
// (the devices of an in-process multi-GPU key are uploaded one after the other from the same descriptor: one transform serves all)
static thread_local bool lagrange_keep_cache = false;
namespace {
struct LagrangeCache {
  const void* q = nullptr;
  size_t used = 0;
  int log_n = -1, curve = -1;
  std::vector<uint64_t> xy;
  std::vector<uint8_t> inf;
  void clear() {
    q = nullptr;
    std::vector<uint64_t>().swap(xy);
    std::vector<uint8_t>().swap(inf);
  }
  // this cache holding the transform (lagrange_h, `mode`) of d's H query: kept from the upload before (KeepLagrange) if it was made
  // from the same query, computed otherwise
  const LagrangeCache& transformed(zkp_ctx* ctx, const zkp_groth16_pk_desc* d, size_t h_used, int lg, int mode) {
    if (!(lagrange_keep_cache && q == d->h_query && used == h_used && log_n == lg && curve == d->curve)) {
      lagrange_h(ctx, d->curve, d->h_query, d->h_inf, h_used, lg, &xy, &inf, mode);
      q = d->h_query;
      used = h_used;
      log_n = lg;
      curve = d->curve;
    }
    return *this;
  }
  // the upload is done with it
  void release() {
    if (!lagrange_keep_cache) clear();
  }
};
thread_local LagrangeCache lagrange_cache, lagrange_cache_g;             // the transformed H query (mode 0) | the bases of the C part (mode 1)
}  // namespace

KeepLagrange::KeepLagrange() { lagrange_keep_cache = true; }
KeepLagrange::~KeepLagrange() {
  lagrange_keep_cache = false;
  lagrange_cache.clear();
  lagrange_cache_g.clear();
}

// mode 1: G_k = (zinv / N) sum_i w^-ik H_i instead (the inverse transform of H itself, scaled by zinv = 1 / Z(g)): the bases of
// the C part of h, see fold_c_into_l below.
static void lagrange_h(zkp_ctx* ctx, int curve, const uint64_t* h_query, const uint8_t* h_inf, size_t h_used, int log_n,
                       std::vector<uint64_t>* xy_out, std::vector<uint8_t>* inf_out, int mode) {
  using namespace hostf;
  const HostField F = fr_field(curve);
  const size_t N = (size_t)1 << log_n, fq = curve == ZKP_BN254 ? 4 : 6;
  const MsmVtbl* v1 = msm_vtbl(curve, 1);
  auto ld = [&](const uint32_t* p) {
    HostField::E e{};
    memcpy(e.data(), p, 32);
    return e;
  };
  const int adicity = curve == ZKP_BN254 ? consts::Bn254Fr::TWO_ADICITY : consts::Bls381Fr::TWO_ADICITY;
  HostField::E wi = ld(curve == ZKP_BN254 ? consts::Bn254Fr::ROOT_INV : consts::Bls381Fr::ROOT_INV);
  const HostField::E gi = ld(curve == ZKP_BN254 ? consts::Bn254Fr::GEN_INV : consts::Bls381Fr::GEN_INV);
  wi = F.pow2k(wi, adicity - log_n);                                   // w_N^-1
  // scal_i = g^-i / N (mode 1: zinv / N for every i), tw_e = w^-e: generated on the device (canonical words) from four Montgomery constants
  HostField::E mult = F.inverse(F.from_u64((uint64_t)N));
  HostField::E sbase = gi;
  if (mode == 1) {                                                     // zinv = 1 / (g^N - 1)
    const HostField::E g = ld(curve == ZKP_BN254 ? consts::Bn254Fr::GEN : consts::Bls381Fr::GEN);
    mult = F.mul(mult, F.inverse(F.sub(F.pow2k(g, log_n), F.one_())));
    sbase = F.one_();
  }
  const HostField::E one = F.one_();
  uint32_t hconst[4 * 8];
  memcpy(hconst, sbase.data(), 32);
  memcpy(hconst + 8, mult.data(), 32);
  memcpy(hconst + 16, wi.data(), 32);
  memcpy(hconst + 24, one.data(), 32);
  hipStream_t st = ctx->cur->stream;
  DevBuf d_xy, d_inf, d_scal, d_tw, d_X, d_oxy, d_oinf;
  const size_t ab = v1->aff_bytes;
  char* xy = d_xy.as<char>(std::max<size_t>(h_used, 1) * ab);
  uint8_t* inf = d_inf.as<uint8_t>(std::max<size_t>(h_used, 1));
  ZKP_REQUIRE(ab == 2 * fq * 8, ZKP_ERR_BAD_ARG);
  if (h_used) ZKP_HIP(hipMemcpyAsync(xy, h_query, h_used * ab, hipMemcpyHostToDevice, st));
  if (h_used && h_inf) ZKP_HIP(hipMemcpyAsync(inf, h_inf, h_used, hipMemcpyHostToDevice, st));
  else ZKP_HIP(hipMemsetAsync(inf, 0, std::max<size_t>(h_used, 1), st));
  const size_t ntw = std::max<size_t>(N / 2, 1);
  uint32_t* dscal = d_scal.as<uint32_t>(N * 8 + 32);
  uint32_t* dtw = d_tw.as<uint32_t>(ntw * 8);
  uint32_t* dconst = dscal + N * 8;
  ZKP_HIP(hipMemcpyAsync(dconst, hconst, sizeof hconst, hipMemcpyHostToDevice, st));
  with_fr(curve, [&](auto P) {
    hipLaunchKernelGGL(pow_canon_kernel<decltype(P)>, dim3((N + 255) / 256), dim3(256), 0, st, dscal, dconst, dconst + 8, (uint32_t)N);
    hipLaunchKernelGGL(pow_canon_kernel<decltype(P)>, dim3((ntw + 255) / 256), dim3(256), 0, st, dtw, dconst + 16, dconst + 24, (uint32_t)ntw);
  });
  char* X = d_X.as<char>(N * v1->bucket_bytes);           // stage points in the bucket (unsaturated) layout
  char* oxy = d_oxy.as<char>(N * ab);
  uint8_t* oinf = d_oinf.as<uint8_t>(N);
  v1->gfft(st, xy, inf, h_used, dscal, dtw, (uint32_t)log_n, X, oxy, oinf);
  ZKP_HIP(hipGetLastError());
  xy_out->resize(N * 2 * fq);
  inf_out->resize(N);
  ZKP_HIP(hipMemcpyAsync(xy_out->data(), oxy, N * ab, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipMemcpyAsync(inf_out->data(), oinf, N, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

// ---- The C matrix folded into the L query (round 4).  The quotient's coefficients are h = coset_ifft(a_c b_c zinv) - zinv C(X) (the
// coset evaluations c_c of C(X) = interpolant of C z go through coset_ifft unchanged), so
//     sum_i h_i H_i = sum_j (a_c b_c zinv)_j H'_j  -  sum_k (C z)_k G_k,      G_k = (zinv / N) sum_i w^-ik H_i
// and the second sum is LINEAR in the assignment: sum_m z_m D_m with D_m = sum_k C_km G_k.  With L'_m = L_m - D_m (inputs: -D_m,
// in the slots that are the identity in the index-aligned L table) the prover needs neither C z nor the ifft -> coset_fft chain
// of c (r1cs_to_qap.rs:155-162): 12 instead of 18 transform passes per proof, for every assignment, satisfying or not.
// fold_c_into_l: the plan (on the host, groth16_fold_plan.hpp), the kernel over the light columns, one MSM per heavy column.

// L'_m = L_m - sum_k C_km G_k over the LIGHT columns of the plan, for every variable m: one lane per variable (v1->lfold)
static void run_fold_kernel(zkp_ctx* ctx, const zkp_groth16_pk_desc* d, size_t nz, const FoldCsc& csc, const std::vector<uint64_t>& g_xy,
                            const std::vector<uint8_t>& g_inf, std::vector<uint64_t>* l_xy, std::vector<uint8_t>* l_inf) {
  const MsmVtbl* v1 = msm_vtbl(d->curve, 1);
  const size_t fq = d->curve == ZKP_BN254 ? 4 : 6, ab = v1->aff_bytes, ni = d->num_inputs;
  // the L query index-aligned with the assignment (leading identities for the inputs)
  std::vector<uint64_t> lq(nz * 2 * fq, 0);
  std::vector<uint8_t> li(nz, 1);
  for (size_t m = ni; m < nz; m++) {
    li[m] = d->l_inf ? d->l_inf[m - ni] : 0;
    if (!li[m]) memcpy(&lq[m * 2 * fq], d->l_query + (m - ni) * 2 * fq, ab);
  }
  hipStream_t st = ctx->cur->stream;
  DevBuf b_l, b_li, b_cp, b_rows, b_kind, b_coeff, b_g, b_gi, b_o, b_oi;
  auto up = [&](DevBuf& b, const void* p, size_t bytes) {
    void* dp = b.get(std::max<size_t>(bytes, 16));
    ZKP_HIP(hipMemcpyAsync(dp, p, bytes, hipMemcpyHostToDevice, st));
    return dp;
  };
  const char* dl = (const char*)up(b_l, lq.data(), lq.size() * 8);
  const uint8_t* dli = (const uint8_t*)up(b_li, li.data(), li.size());
  const uint32_t* dcp = (const uint32_t*)up(b_cp, csc.col_ptr.data(), csc.col_ptr.size() * 4);
  const uint32_t* drows = (const uint32_t*)up(b_rows, csc.rows.data(), csc.rows.size() * 4);
  const uint8_t* dkind = (const uint8_t*)up(b_kind, csc.kind.data(), csc.kind.size());
  const uint32_t* dcoeff = (const uint32_t*)up(b_coeff, csc.coeff.data(), csc.coeff.size() * 4);
  const char* dg = (const char*)up(b_g, g_xy.data(), g_xy.size() * 8);
  const uint8_t* dgi = (const uint8_t*)up(b_gi, g_inf.data(), g_inf.size());
  char* o = (char*)b_o.get(nz * ab);
  uint8_t* oi = (uint8_t*)b_oi.get(nz);
  v1->lfold(st, dl, dli, nz, dcp, drows, dkind, dcoeff, dg, dgi, o, oi);
  ZKP_HIP(hipGetLastError());
  l_xy->resize(nz * 2 * fq);
  l_inf->resize(nz);
  ZKP_HIP(hipMemcpyAsync(l_xy->data(), o, nz * ab, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipMemcpyAsync(l_inf->data(), oi, nz, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

// L'_m = L_m - D_m for the HEAVY columns m of the plan, D_m = one MSM over column m.  A column's (row, entry) list is given up as
// soon as its MSM has run.
static void subtract_heavy_columns(zkp_ctx* ctx, const zkp_groth16_pk_desc* d, FoldCsc& csc, const std::vector<uint64_t>& g_xy,
                                   const std::vector<uint8_t>& g_inf, std::vector<uint64_t>* l_xy, std::vector<uint8_t>* l_inf) {
  using namespace hostf;
  const std::vector<uint32_t>& heavy_cols = csc.heavy_cols;
  if (heavy_cols.empty()) return;
  const HostField Q = fq_field(d->curve);
  const size_t fq = d->curve == ZKP_BN254 ? 4 : 6;
  const size_t fw = 2 * fq;                                  // u64 words of an affine point
  std::vector<HostJac> res(heavy_cols.size());
  std::vector<uint64_t> xyz(3 * fq);
  std::vector<uint64_t> cxy, csc_;
  std::vector<uint8_t> cinf;
  for (size_t i = 0; i < heavy_cols.size(); i++) {
    const uint32_t m = heavy_cols[i];
    const size_t cn = csc.heavy[i].size();
    cxy.resize(cn * fw);
    csc_.resize(cn * 4);
    cinf.resize(cn);
    for (size_t j = 0; j < cn; j++) {
      const uint32_t k = csc.heavy[i][j].first, e = csc.heavy[i][j].second;
      memcpy(&cxy[j * fw], &g_xy[(size_t)k * fw], 8 * fw);
      cinf[j] = g_inf[k];
      memcpy(&csc_[j * 4], d->ct.coeff + (size_t)e * 4, 32);
    }
    std::vector<std::pair<uint32_t, uint32_t>>().swap(csc.heavy[i]);
    msm_var_run(ctx, d->curve, 1, cxy.data(), cinf.data(), csc_.data(), cn, /*montgomery=*/true, xyz.data());
    HostJac D = host_jac_load(Q, xyz.data());
    D.y = Q.neg(D.y);
    HostJac Lm{};
    if ((*l_inf)[m]) {
      Lm.x = Q.one_();
      Lm.y = Q.one_();
    } else {
      memcpy(Lm.x.data(), l_xy->data() + (size_t)m * fw, 8 * fq);
      memcpy(Lm.y.data(), l_xy->data() + (size_t)m * fw + fq, 8 * fq);
      Lm.z = Q.one_();
    }
    res[i] = host_jac_add(Q, Lm, D);
  }
  std::vector<uint64_t> axy(heavy_cols.size() * fw);
  std::vector<uint8_t> ainf(heavy_cols.size());
  host_into_affine(Q, res, axy.data(), fw, ainf.data());
  for (size_t i = 0; i < heavy_cols.size(); i++) {
    memcpy(l_xy->data() + (size_t)heavy_cols[i] * fw, axy.data() + i * fw, 8 * fw);
    (*l_inf)[heavy_cols[i]] = ainf[i];
  }
}

static void fold_c_into_l(zkp_ctx* ctx, const zkp_groth16_pk_desc* d, size_t nz, const std::vector<uint64_t>& g_xy,
                          const std::vector<uint8_t>& g_inf, std::vector<uint64_t>* l_xy, std::vector<uint8_t>* l_inf) {
  const hostf::HostField F = hostf::fr_field(d->curve);
  const hostf::HostField::E one = F.one_(), minus_one = F.neg(one);
  const zkp_csr& c = d->ct;
  const std::vector<uint64_t> costs = fold_column_costs(nz, c.row_ptr[d->num_constraints], c.col, c.coeff, one.data(), minus_one.data());
  // the cut chosen per key unless zkp_ctx_config.c_fold_heavy_cost / ZKP_LFOLD_HEAVY_COST fixes it
  const uint64_t cut = fold_heavy_cut(costs, ctx->cfg.lfold_heavy_cost > 0 ? (uint64_t)ctx->cfg.lfold_heavy_cost : 0);
  FoldCsc csc;
  ZKP_REQUIRE(fold_build_csc(nz, d->num_constraints, c.row_ptr, c.col, c.coeff, one.data(), minus_one.data(), costs, cut, &csc),
              ZKP_ERR_BAD_ARG);
  run_fold_kernel(ctx, d, nz, csc, g_xy, g_inf, l_xy, l_inf);
  subtract_heavy_columns(ctx, d, csc, g_xy, g_inf, l_xy, l_inf);
}

// ---- One key upload, phase by phase in the order groth16_pk_upload lists them.  Every query table is resident when its phase
// returns; the key under construction is released with everything it names if a phase throws.
// flags bit 0 (zkp_groth16_pk_upload_ex, ZKP_PK_KEEP_FORM): the key as given.  rank / world: the slice of a base-sharded key.
namespace {
struct KeyBuild {
  zkp_ctx* const ctx;
  const zkp_groth16_pk_desc* const d;
  const int rank, world, flags;
  struct Release {
    zkp_ctx* ctx;
    void operator()(zkp_groth16_pk* p) const { groth16_pk_free(ctx, p); }     // a partly built key: zero handles and null pointers are skipped
  };
  std::unique_ptr<zkp_groth16_pk, Release> pk;
  const bool matrices_only;
  const size_t fq;
  const uint64_t* const tA[4];           // the tail points behind each query (file comment of groth16.hip), nullptr = identity
  const uint64_t* const tB1[4];
  const uint64_t* const tB2[4];
  const uint64_t* const tL[4];
  // what a phase leaves for the phases behind it
  size_t h_used = 0;                     // the min(h_len, N) terms of the H query the MSM actually uses (prover.rs:186-187)
  size_t h_table_n = 0;                  // points of this rank's H table (plan_slices)
  bool lagrange_on = false;              // the H query goes to evaluation form (plan_slices)
  int lgk = 0;                           // window-group size of the whole key
  int cB = 0, capB = 0;                  // window bits / task cap of the B queries, 0 = the key's (plan_b_window)
  std::vector<uint8_t> fA, fB1, fB2, fL; // identity flags of the uploaded slices
  size_t al_differ = 0;                  // bases that are the identity in exactly one of A and L (plan_al_sort)

  static zkp_groth16_pk* checked(const zkp_groth16_pk_desc* d, int rank, int world) {
    ZKP_REQUIRE(d->curve == ZKP_BN254 || d->curve == ZKP_BLS12_381, ZKP_ERR_UNSUPPORTED_CURVE);
    ZKP_REQUIRE(d->num_inputs >= 1, ZKP_ERR_BAD_ARG);
    ZKP_REQUIRE(world >= 0 && (world == 0 ? rank == 0 : (rank >= 0 && rank < world)), ZKP_ERR_BAD_ARG);
    return new zkp_groth16_pk();
  }
  KeyBuild(zkp_ctx* ctx, const zkp_groth16_pk_desc* d, int rank, int world, int flags)
      : ctx(ctx), d(d), rank(rank), world(world), flags(flags), pk(checked(d, rank, world), Release{ctx}),
        matrices_only(d->a_query == nullptr), fq(d->curve == ZKP_BN254 ? 4 : 6), tA{d->alpha_g1, d->delta_g1, nullptr, nullptr},
        tB1{d->beta_g1, nullptr, d->delta_g1, nullptr}, tB2{d->beta_g2, nullptr, d->delta_g2, nullptr},
        tL{nullptr, nullptr, nullptr, d->delta_g1} {
    pk->shard_rank = rank;
    pk->shard_world = world;
    pk->curve = d->curve;
    pk->num_inputs = d->num_inputs;
    pk->num_aux = d->num_aux;
    pk->num_constraints = d->num_constraints;
    pk->nz = (size_t)d->num_inputs + d->num_aux;
    size_t dom = (size_t)d->num_constraints + d->num_inputs;       // r1cs_to_qap.rs:123-126
    int lg = 0;
    while (((size_t)1 << lg) < dom) lg++;
    ZKP_REQUIRE(lg <= (d->curve == ZKP_BN254 ? 28 : 32) && lg <= 30, ZKP_ERR_DOMAIN_TOO_LARGE);
    pk->log_n = lg;
    pk->N = (size_t)1 << lg;
    if (!matrices_only) {
      ZKP_REQUIRE(d->a_len == pk->nz && d->b_g1_len == pk->nz && d->b_g2_len == pk->nz, ZKP_ERR_BAD_ARG);
      ZKP_REQUIRE(d->l_len == d->num_aux, ZKP_ERR_BAD_ARG);
    }
    ZKP_REQUIRE(!(matrices_only && world > 0), ZKP_ERR_BAD_ARG);       // a matrices-only key has no queries to shard
  }

  void upload_matrices() {
    pk->m[0] = upload_csr(ctx, d->at, d->num_constraints);
    pk->m[1] = upload_csr(ctx, d->bt, d->num_constraints);
    pk->m[2] = upload_csr(ctx, d->ct, d->num_constraints);
  }

  // slice of every query this rank keeps resident (everything for an unsharded key), the form of the H query and the window-group
  // size of the whole key
  void plan_slices() {
    for (auto p : {d->alpha_g1, d->beta_g1, d->delta_g1, d->beta_g2, d->delta_g2}) ZKP_REQUIRE(p, ZKP_ERR_BAD_ARG);
    h_used = std::min<size_t>(d->h_len, pk->N);
    shard_bounds(pk->nz + 4, rank, world, &pk->q_lo[0], &pk->q_n[0]);
    pk->q_lo[1] = pk->q_lo[2] = pk->q_lo[0];
    pk->q_n[1] = pk->q_n[2] = pk->q_n[0];
    // L is stored index-aligned with z (num_inputs leading identity points): its MSM then runs over the same scalar
    // slice as A / B1 / B2 and can reuse their bucket sort
    pk->q_lo[4] = pk->q_lo[0];
    pk->q_n[4] = pk->q_n[0];
    // ONE predicate for "the H query goes to evaluation form" (the planning block and the upload below used to evaluate two
    // different ones): flags bit 0 (zkp_groth16_pk_upload_ex, ZKP_PK_KEEP_FORM) keeps the key as given — no group transforms at upload
    // (one-shot and low-volume callers: the transforms cost ~0.65 s per 2^20 and pay back after ~2000 proofs), 7 transforms per proof;
    // zkp_ctx_config.h_evaluation_form / ZKP_H_LAGRANGE switches it per context.
    lagrange_on = ctx->cfg.h_lagrange && !(flags & 1) && d->h_query && h_used > 0 && pk->log_n >= 1;
    // The H slice is cut from the min(h_len, N) terms the MSM actually uses (prover.rs:186-187)
    // (the evaluation-form H query has N points, one more than the h_len = N - 1 the reference keeps: ADVICE r4; a sharded key
    //  re-shards it over N, so its slice is planned from N as well)
    // The only place that computes it: upload_h uploads what is planned here.  An unsharded key in coefficient form keeps the query
    // at its given length.
    shard_bounds(lagrange_on ? pk->N : h_used, rank, world, &pk->q_lo[3], &pk->q_n[3]);
    h_table_n = lagrange_on || world > 0 ? pk->q_n[3] : (size_t)d->h_len;
    // Window-group size for the WHOLE key (msm.hip BasesEntry::lgk): the five queries are sized together so that they keep one
    // window configuration (sort sharing) and their tables fit ZKP_TABLE_BUDGET_GB / the free device memory.
    const int groups[5] = {1, 1, 2, 1, 1};
    const size_t ns[5] = {pk->q_n[0], pk->q_n[1], pk->q_n[2], h_table_n, pk->q_n[4]};
    lgk = bases_plan_lgk(ctx, d->curve, groups, ns, 5);
    if (lgk > 0 && env_str("ZKP_DEBUG_MSM")) fprintf(stderr, "[groth16] window tables do not fit: window groups of %d\n", 1 << lgk);
  }

  // Window bits of the B queries (round 3).  A G2 bucket costs two Fq2 point additions in the reduction against 6 mixed
  // additions' worth of accumulate per entry, and half of a typical B query are identity points: with the c = round(log2 n) of
  // the G1 queries the B2 reduction (2^19 buckets) cost 0.70 ms per 2^20 proof beside 1.30 ms of accumulate.  Sized by the LIVE
  // bases, c = round(log2 live) - 2 (17 for the MiMC chain: 15 windows, 2^16 buckets, tasks of <= 32 entries so that the
  // accumulate kernel still fills the machine).  B1 takes the same configuration so that it keeps reusing B2's bucket sort.
  void plan_b_window() {
    // Measured (2^20 MiMC chain, same box): B2 MSM 3.72 -> 3.27-3.45 ms standalone, but the B queries then leave the shared
    // level-1 pass (one more digit scan per proof) and their accumulate kernels run 18-30 % longer instead of the 15 % more
    // entries: 139.2 (c = 17), 139.8 (c = 18), 137.2 (c = 16) vs 139.9 proofs/s with the shared configuration.  Off by
    // default; ZKP_B_WINDOW=1 enables it (ZKP_B_WINDOW_BITS / ZKP_B_TASK_CAP override the choice).
    size_t live = 0;
    for (size_t i = 0; i < d->b_g2_len; i++) live += !(d->b_g2_inf && d->b_g2_inf[i]);
    int lg2 = 0;
    while (((size_t)2 << lg2) <= std::max<size_t>(live, 1)) lg2++;
    if (lg2 < 62 && (double)live >= 1.41421356 * (double)((size_t)1 << lg2)) lg2++;
    const zkp_tune& tune = ctx->tune;                      // b_window_bits / b_task_cap: -1 = not given
    if (tune.b_window && world == 0 && live >= ((size_t)1 << 14) && !ctx->cfg.msm_c && !ctx->cfg.msm_c_g2) {
      cB = tune.b_window_bits >= 0 ? tune.b_window_bits : std::max(12, std::min(20, lg2 - 2));
      capB = tune.b_task_cap >= 0 ? tune.b_task_cap : 32;
    }
  }

  void upload_a_b() {
    pk->hA = upload_ext(ctx, d->curve, 1, d->a_query, d->a_inf, d->a_len, 2 * fq, tA, pk->q_lo[0], pk->q_n[0], 0, &fA, 0, 0, lgk);
    pk->hB1 = upload_ext(ctx, d->curve, 1, d->b_g1_query, d->b_g1_inf, d->b_g1_len, 2 * fq, tB1, pk->q_lo[1], pk->q_n[1], 0, &fB1, cB, capB, lgk);
    pk->hB2 = upload_ext(ctx, d->curve, 2, d->b_g2_query, d->b_g2_inf, d->b_g2_len, 4 * fq, tB2, pk->q_lo[2], pk->q_n[2], 0, &fB2, cB, capB, lgk);
    // B1 reuses B2's bucket sort + task schedule (same scalars, window configuration and identity pattern): -0.55 ms of
    // memory-bound sort kernels per proof.  With 4 hardware queues this LOST 2 % (84.7 -> 83.0 proofs/s: the wait on
    // B2's stream idled a queue); with 16 queues it gains 1-2 % (97.9 -> 99.3).  ZKP_SHARE_B_SORT=0 disables it.
    const bool same_inf = (!d->b_g1_inf && !d->b_g2_inf) ||
                          (d->b_g1_inf && d->b_g2_inf && memcmp(d->b_g1_inf, d->b_g2_inf, d->b_g1_len) == 0);
    pk->share_b_sort = ctx->tune.share_b_sort && same_inf && bases_same_shape(ctx, pk->hB1, pk->hB2);
  }

  // this rank's slice (plan_slices) of the H query: of its evaluation form, or of the query as given
  void upload_h() {
    if (lagrange_on) {
      const LagrangeCache& cache = lagrange_cache.transformed(ctx, d, h_used, pk->log_n, 0);
      pk->hH = bases_upload(ctx, d->curve, 1, cache.xy.data() + pk->q_lo[3] * 2 * fq, cache.inf.data() + pk->q_lo[3], h_table_n, 0, 0, lgk);
      pk->h_lagrange = true;
      lagrange_cache.release();
    } else {
      pk->hH = bases_upload(ctx, d->curve, 1, d->h_query ? d->h_query + pk->q_lo[3] * 2 * fq : nullptr,
                            d->h_inf ? d->h_inf + pk->q_lo[3] : nullptr, h_table_n, 0, 0, lgk);
    }
  }

  // the L query with C folded into it (an evaluation-form key, unless zkp_ctx_config.c_fold / ZKP_C_FOLD is off), or as given
  void upload_l() {
    if (pk->h_lagrange && ctx->cfg.c_fold && d->l_query) {
      std::vector<uint64_t> lxy;
      std::vector<uint8_t> linf;
      const LagrangeCache& gc = lagrange_cache_g.transformed(ctx, d, h_used, pk->log_n, 1);
      fold_c_into_l(ctx, d, pk->nz, gc.xy, gc.inf, &lxy, &linf);          // the whole L'; upload_ext keeps this rank's slice
      lagrange_cache_g.release();
      pk->hL = upload_ext(ctx, d->curve, 1, lxy.data(), linf.data(), pk->nz, 2 * fq, tL, pk->q_lo[4], pk->q_n[4], 0, &fL, 0, 0, lgk);
      pk->c_folded = true;
    } else {
      pk->hL = upload_ext(ctx, d->curve, 1, d->l_query, d->l_inf, d->l_len, 2 * fq, tL, pk->q_lo[4], pk->q_n[4],
                          d->num_inputs, &fL, 0, 0, lgk);
    }
  }

  // L reuses A's bucket sort + task schedule (L is stored index-aligned with z, so both MSMs run over the same scalar
  // slice): one digit scan + level-2 sort + schedule less per proof.  The shared sort drops a base only if it is the
  // identity in BOTH queries (A's scan then uses the intersection of the two flag vectors, bases_set_sort_flags); a base
  // that is the identity in one query only stays in the list and the accumulate kernel skips it when it gathers it.
  // That is only worth it when such bases are rare: a lane whose point is the identity idles while its wave-mates add
  // (measured: B2 sharing a full-pattern sort ran 4.47 instead of 1.91 ms — half of the MiMC chain's B-query is
  // identities).  In the MiMC chain A and L each have ~210 K identity bases of 1.26 M that the other does not: sharing
  // made both accumulate kernels 20 % longer (1.02 -> 1.25 ms) for one sort less, 122.2 vs 121.0 proofs/s and + 0.2 ms
  // single-proof latency — not taken: the limit is 1/16 of the bases.
  // ZKP_SHARE_AL_SORT=0 disables it.
  void plan_al_sort() {
    bool same = fA.size() == fL.size() && pk->q_lo[0] == pk->q_lo[4];
    std::vector<uint8_t> both(fA.size());
    for (size_t k = 0; same && k < fA.size(); k++) {
      both[k] = fA[k] & fL[k];
      al_differ += fA[k] != fL[k];
    }
    pk->share_al_sort = ctx->tune.share_al_sort && same && al_differ <= fA.size() / 16 && bases_same_shape(ctx, pk->hL, pk->hA) && pk->q_n[0] > 0;
    if (pk->share_al_sort && al_differ) bases_set_sort_flags(ctx, pk->hA, both.data(), both.size());
  }

  // One level-1 pass over z for A, B2 (whose sort B1 reuses) and L: the digit scan, the (bin, tile) counts and the scatter
  // into bins are done once, by A, over the bases that are NOT the identity in all three queries; every query then
  // runs its own level-2 sort and drops its own identities there (three flag bits in the top of every entry, bases_set_group), so
  // each accumulate kernel still sees exactly its own entries.  Two of the four digit scans of a proof disappear
  // (ZKP_SHARE_L1=0 disables it).
  void plan_shared_level1() {
    const bool aligned = fA.size() == fL.size() && fA.size() == fB2.size() && pk->q_lo[0] == pk->q_lo[4] &&
                         pk->q_lo[0] == pk->q_lo[2] && pk->q_n[0] > 0;
    if (!(ctx->tune.share_l1 && aligned && !pk->share_al_sort && bases_same_shape(ctx, pk->hL, pk->hA))) return;
    // (hB2 is a G2 table: same n, window configuration checked through hB1 / share_b_sort).  B queries with their own
    // window configuration (plan_b_window) run their own level-1 pass: the group is then A and L only.
    const bool with_b = pk->share_b_sort && bases_same_shape(ctx, pk->hB1, pk->hA);
    std::vector<uint8_t> all(fA.size()), member(fA.size());
    for (size_t k = 0; k < fA.size(); k++) {
      all[k] = fA[k] & fL[k] & (with_b ? fB2[k] : (uint8_t)1);
      member[k] = all[k] ? 0 : (uint8_t)((fA[k] ? 1 : 0) | (with_b && fB2[k] ? 2 : 0) | (fL[k] ? 4 : 0));
    }
    bases_set_sort_flags(ctx, pk->hA, all.data(), all.size());
    bases_set_group(ctx, pk->hA, member.data(), member.size());
    bases_set_filter_bit(ctx, pk->hA, 0);
    if (with_b) bases_set_filter_bit(ctx, pk->hB2, 1);
    bases_set_filter_bit(ctx, pk->hL, 2);
    pk->share_l1 = true;
    pk->b_in_l1 = with_b;
  }

  // C only ever needs l' + h_acc (prover.rs:189-196): with equal bucket ranges and no window groups H's accumulate kernel
  // continues from L's finished buckets and ONE reduction yields the sum; L's own result is the identity (ZKP_CHAIN_LH=0: off)
  void plan_chain_lh() {
    uint64_t iL[5], iH[5];
    bases_info(ctx, pk->hL, iL);
    bases_info(ctx, pk->hH, iH);
    pk->chain_lh = ctx->tune.chain_lh && iL[0] == iH[0] && iL[2] == 1 && iH[2] == 1 && pk->q_n[3] > 0 && pk->q_n[4] > 0;
  }

  // which sorts and passes the prover's five MSMs share
  void plan_sharing() {
    plan_al_sort();
    plan_shared_level1();
    plan_chain_lh();
    if (env_str("ZKP_DEBUG_MSM"))
      fprintf(stderr, "[groth16] A/L sort sharing: %d (flags differ at %zu of %zu bases), B1/B2: %d, shared level 1: %d\n",
              (int)pk->share_al_sort, al_differ, fA.size(), (int)pk->share_b_sort, (int)pk->share_l1);
  }

  // the witness map's constant, the buffers of the first two lanes; -> the finished key, which the caller owns
  zkp_groth16_pk* finish() {
    uint32_t* consts = pk->consts.as<uint32_t>(64);
    const int lg = pk->log_n;
    with_fr(d->curve, [&](auto P) { hipLaunchKernelGGL(qap_consts_kernel<decltype(P)>, dim3(1), dim3(64), 0, ctx->cur->stream, consts, lg); });
    ZKP_HIP(hipGetLastError());
    for (int l = 0; l < 2; l++) {                     // further lanes allocate on first use
      auto& L = pk->lane[l];
      L.abc.get(3 * pk->N * 32);
      L.S.get((pk->nz + 4) * 32);
      L.results.get(6 * 16 * 24 * 4 + 64);
      L.proof.get(4096);
    }
    ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));
    return pk.release();
  }
};
}  // namespace

zkp_groth16_pk* groth16_pk_upload(zkp_ctx* ctx, const zkp_groth16_pk_desc* d, int rank, int world, int flags) {
  KeyBuild key(ctx, d, rank, world, flags);
  key.upload_matrices();
  if (!key.matrices_only) {
    key.plan_slices();
    key.plan_b_window();
    key.upload_a_b();
    key.upload_h();
    key.upload_l();
    key.plan_sharing();
  }
  return key.finish();
}

// also the release of a partly built key (KeyBuild): zero handles and null pointers are skipped
void groth16_pk_free(zkp_ctx* ctx, zkp_groth16_pk* pk) {
  (void)hipDeviceSynchronize();
  for (auto& PL : pk->lane) {
    if (PL.graph_exec) (void)hipGraphExecDestroy(PL.graph_exec);
    if (PL.graph) (void)hipGraphDestroy(PL.graph);
  }
  for (uint64_t h : {pk->hA, pk->hB1, pk->hB2, pk->hH, pk->hL})
    if (h) bases_drop(ctx, h);
  for (auto& m : pk->m) {
    if (m.row_ptr) (void)hipFree(m.row_ptr);
    if (m.col) (void)hipFree(m.col);
    if (m.coeff) (void)hipFree(m.coeff);
  }
  delete pk;
}

uint64_t groth16_domain_size(zkp_groth16_pk* pk) { return pk->N; }
void groth16_pk_info(zkp_ctx* ctx, zkp_groth16_pk* pk, uint64_t info[8]) {
  for (int i = 0; i < 8; i++) info[i] = 0;
  if (!pk->hA) return;
  uint64_t a[5], b[5];
  bases_info(ctx, pk->hA, a);
  bases_info(ctx, pk->hB2, b);
  info[0] = a[2];
  for (uint64_t h : {pk->hA, pk->hB1, pk->hB2, pk->hH, pk->hL}) {
    uint64_t t[5];
    bases_info(ctx, h, t);
    info[1] += t[4];
  }
  info[2] = a[0];
  info[3] = a[1];
  info[4] = a[3];
  info[5] = b[0];
  info[6] = (pk->share_b_sort ? 1 : 0) | (pk->share_al_sort ? 2 : 0) | (pk->share_l1 ? 4 : 0) | (pk->fused_groups << 32);
  info[7] = (pk->h_lagrange ? 1 : 0) | (pk->c_folded ? 2 : 0) | (pk->chain_lh ? 4 : 0);       // key form (slots L / H)
}

}  // namespace zkp
