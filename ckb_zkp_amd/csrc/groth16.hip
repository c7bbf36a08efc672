// Groth16 prover orchestration on the device: the host-side mirror of
// /root/reference/groth16/src/prover.rs:124-211 (`create_proof`) and
// /root/reference/groth16/src/r1cs_to_qap.rs:113-172 (`R1CStoQAP::witness_map`).
//
// What stays on the caller's side: circuit synthesis (Rust closures filling `ProvingAssignment`,
// prover.rs:16-95).  What crosses the boundary: the three sparse matrices at/bt/ct (fixed per circuit,
// uploaded with the key) and the full assignment z = input_assignment ++ aux_assignment (Montgomery Fr).
//
// Device pipeline for one proof (everything resident in HBM, one stream, no host round trips until the
// 3 proof points come back):
//   1. a,b,c = A z, B z, C z (CSR, one lane per constraint row)            r1cs_to_qap.rs:131-142,154-159
//   2. ifft, coset_fft on a,b,c; ab = (a*b - c) / Z(g); coset_ifft -> h     r1cs_to_qap.rs:144-169
//   3. five MSMs; `into_repr()` (prover.rs:150-161) is fused into the MSM digit scan
//   4. assemble A, B, C                                                      prover.rs:164-210
//
// Restructuring that keeps the result identical (a proof is three group elements, so any evaluation order
// is bit-exact): the small fixed-point terms of prover.rs:165-177,183,213-228 are folded INTO the MSMs by
// extending each query with a few key points and the scalar vector with (1, r, s, -rs):
//     S      = z ++ [1, r, s, -r*s]
//     A_ext  = a_query    ++ [alpha_g1, delta_g1, inf,      inf     ]   -> g_a  = <A_ext , S>
//     B1_ext = b_g1_query ++ [beta_g1 , inf,      delta_g1, inf     ]   -> g1_b = <B1_ext, S>
//     B2_ext = b_g2_query ++ [beta_g2 , inf,      delta_g2, inf     ]   -> g2_b = <B2_ext, S>
//     L_ext  = l_query    ++ [inf,      inf,      inf,      delta_g1]   -> l'   = <L_ext , S[num_inputs..]>
// (z[0] = 1 so query[0] needs no special case; r == 0 makes r*g1_b the identity exactly as the reference's
// `if r != 0` branch does).  What remains is  C = s*g_a + r*g1_b + l' + h_acc  and three `into_affine()`.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "field_dev.hpp"
#include "fr_dev.hpp"              // with_fr: only ever reached with the curve of an uploaded key, its throw is unreachable here
#include "groth16_pk.hpp"
#include "host_field.hpp"
#include "internal.hpp"
#include "msm_vtbl.hpp"

using namespace zkp;

namespace zkp {

// a[row] = sum coeff * z[col] ; rows >= num_constraints: a gets z[row - nc] for the next num_inputs rows, 0 after
template <class P>
__global__ __launch_bounds__(256) void csr_eval_kernel(const uint32_t* __restrict__ row_ptr,
                                                       const uint32_t* __restrict__ col,
                                                       const uint32_t* __restrict__ coeff,
                                                       const uint32_t* __restrict__ z, uint32_t nc, uint32_t N,
                                                       uint32_t num_inputs, int is_a, uint32_t* __restrict__ out) {
  using F = Fp<P>;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  F acc = F::zero();
  if (i < nc) {
    const F one = F::one();
    for (uint32_t k = row_ptr[i]; k < row_ptr[i + 1]; k++) {
      F v = F::load(z + (size_t)col[k] * 8);
      F cf = F::load(coeff + (size_t)k * 8);
      if (cf == one) acc = acc + v;          // evaluate_constraint's is_one fast path (r1cs_to_qap.rs:39-43)
      else acc = acc + v * cf;
    }
  } else if (is_a && i - nc < num_inputs) {
    acc = F::load(z + (size_t)(i - nc) * 8); // r1cs_to_qap.rs:140-142
  }
  acc.store(out + (size_t)i * 8);
}

// ab[i] = (a[i]*b[i] - c[i]) * zinv      (r1cs_to_qap.rs:150,164-168)
template <class P>
__global__ __launch_bounds__(256) void qap_pointwise_kernel(uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                            const uint32_t* __restrict__ c,
                                                            const uint32_t* __restrict__ zinv, uint32_t N) {
  using F = Fp<P>;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  F x = F::load(a + (size_t)i * 8) * F::load(b + (size_t)i * 8) - F::load(c + (size_t)i * 8);
  (x * F::load(zinv)).store(a + (size_t)i * 8);
}

// a[i] = a[i]*b[i] * zinv: the pointwise step of a key with C folded into its L query (fold_c_into_l)
template <class P>
__global__ __launch_bounds__(256) void qap_pointwise_ab_kernel(uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                               const uint32_t* __restrict__ zinv, uint32_t N) {
  using F = Fp<P>;
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  (F::load(a + (size_t)i * 8) * F::load(b + (size_t)i * 8) * F::load(zinv)).store(a + (size_t)i * 8);
}

// S tail: [1, r, s, -r*s]
template <class P>
__global__ void scalar_tail_kernel(uint32_t* tail, const uint32_t* rs, size_t tail_step) {
  if (threadIdx.x) return;
  tail += (size_t)blockIdx.x * tail_step;                  // one workgroup per proof of a fused group: tails tail_step, [r, s] 16 words apart
  rs += (size_t)blockIdx.x * 16;
  using F = Fp<P>;
  F r = F::load(rs), s = F::load(rs + 8);
  F::one().store(tail);
  r.store(tail + 8);
  s.store(tail + 16);
  (r * s).neg().store(tail + 24);
}

// ---- the witness map in the pieces both provers compose (groth16_pk.hpp), each on the current stream of ctx.  a | b | c are the
// three N-element thirds of one abc region of a lane; chain k = 0 / 1 / 2 is A z / B z / C z and works in the k-th of them.
void witness_eval(zkp_ctx* ctx, const zkp_groth16_pk* pk, const uint32_t* z_dev, int k, uint32_t* out) {
  const uint32_t N = (uint32_t)pk->N;
  with_fr(pk->curve, [&](auto P) {
    hipLaunchKernelGGL(csr_eval_kernel<decltype(P)>, dim3((N + 255) / 256), dim3(256), 0, ctx->cur->stream, pk->m[k].row_ptr,
                       pk->m[k].col, pk->m[k].coeff, z_dev, pk->num_constraints, N, pk->num_inputs, k == 0 ? 1 : 0, out);
  });
}

// ifft -> coset_fft as one chain of passes (1/N folded into the coset table, no odd-pass copies); falls back to the two
// separate transforms above the full-table domain limit
void witness_transform(zkp_ctx* ctx, const zkp_groth16_pk* pk, uint32_t* buf) {
  if (ntt_ifft_coset_fft(ctx, pk->curve, buf, pk->log_n)) return;
  ntt_run(ctx, pk->curve, buf, pk->log_n, ZKP_NTT_IFFT);
  ntt_run(ctx, pk->curve, buf, pk->log_n, ZKP_NTT_COSET_FFT);
}

// (a, b, c) on the coset -> h, which it returns (it lands in a or b).  coeffs: h in coefficient form wanted
// (zkp_groth16_witness_map; the prover of a coefficient-form key); false with an evaluation-form key: the pointwise values v on the
// coset, the scalars of its H MSM
uint32_t* witness_finish(zkp_ctx* ctx, zkp_groth16_pk* pk, uint32_t* a, bool coeffs) {
  const uint32_t N = (uint32_t)pk->N;
  uint32_t* b = a + pk->N * 8;
  uint32_t* c = b + pk->N * 8;
  const uint32_t* zinv = pk->consts.as<uint32_t>(64);
  hipStream_t st = ctx->cur->stream;
  uint32_t* h = a;
  with_fr(pk->curve, [&](auto P) {
    using FrP = decltype(P);
    if (!coeffs && pk->c_folded) {
      hipLaunchKernelGGL(qap_pointwise_ab_kernel<FrP>, dim3((N + 255) / 256), dim3(256), 0, st, a, b, zinv, N);
    } else if (!coeffs) {
      hipLaunchKernelGGL(qap_pointwise_kernel<FrP>, dim3((N + 255) / 256), dim3(256), 0, st, a, b, c, zinv, N);
    } else if (uint32_t* hq = ntt_qap_coset_ifft(ctx, pk->curve, a, b, c, zinv, pk->log_n)) {
      h = hq;                                            // (a*b - c) / Z(g) fused into the first pass of coset_ifft
    } else {
      hipLaunchKernelGGL(qap_pointwise_kernel<FrP>, dim3((N + 255) / 256), dim3(256), 0, st, a, b, c, zinv, N);
      ntt_run(ctx, pk->curve, a, pk->log_n, ZKP_NTT_COSET_IFFT);
    }
  });
  ZKP_HIP(hipGetLastError());
  return h;
}

// z_dev: nz Fr (device).  Leaves h (N Fr, Montgomery) in the lane's abc and returns it; coeffs as for witness_finish.
// g, G: proof g of a fused group of G (ProofJob) works in the g-th of G abc regions of the lane
uint32_t* witness_map_dev(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint32_t* z_dev, bool coeffs, int g, int G) {
  uint32_t* a = pk->lane[ctx->cur_idx].abc.as<uint32_t>(3 * pk->N * 8 * (size_t)G) + (size_t)g * 3 * pk->N * 8;
  uint32_t* bufs[3] = {a, a + pk->N * 8, a + 2 * pk->N * 8};
  const int nchain = (!coeffs && pk->c_folded) ? 2 : 3;            // C folded into the L query: no C z, no c chain
  for (int k = 0; k < nchain; k++) witness_eval(ctx, pk, z_dev, k, bufs[k]);
  // One launch for a, b, c (grid.y = 3) shortens the witness map in isolation (1.49 -> 1.35 ms at 2^20) but its 3x larger
  // launches delay the MSM streams of the other lane: 79 vs 85 proofs/s pipelined.  Off unless ZKP_NTT_BATCH=1.
  if (ctx->tune.ntt_batch) {
    ntt_run_batch(ctx, pk->curve, bufs, nchain, pk->log_n, ZKP_NTT_IFFT);
    ntt_run_batch(ctx, pk->curve, bufs, nchain, pk->log_n, ZKP_NTT_COSET_FFT);
  } else {
    for (int k = 0; k < nchain; k++) witness_transform(ctx, pk, bufs[k]);
  }
  return witness_finish(ctx, pk, a, coeffs);
}

void groth16_witness_map(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint64_t* z, uint64_t* h, bool on_device) {
  const uint32_t* zd = reinterpret_cast<const uint32_t*>(z);
  if (!on_device) {
    uint32_t* s = pk->lane[ctx->cur_idx].S.as<uint32_t>((pk->nz + 4) * 8);
    ZKP_HIP(hipMemcpyAsync(s, z, pk->nz * 32, hipMemcpyHostToDevice, ctx->cur->stream));
    zd = s;
  }
  uint32_t* hd = witness_map_dev(ctx, pk, zd);
  ZKP_HIP(hipMemcpyAsync(h, hd, pk->N * 32, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->cur->stream));
  if (!on_device) ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));
}

// ---- the buffers of the prove path: each layout is built in one place, by the code that writes it and by the code that reads it ----
constexpr size_t MAX_FN1 = 12, MAX_FN2 = 24;   // 32-bit words of a G1 / G2 coordinate on the largest curve (BLS12-381; MsmVtbl::fN)
constexpr size_t RS_STEP = 16;                 // words between the [r, s] pairs of two proofs (scalar_tail_kernel, assemble_g1_part1)
constexpr size_t FLAG_STEP = 4;                // words between the identity flags of two proofs (three are used)

// 32-bit words of the three proof points (A and C in G1, B in G2).  The proof as it is handed out: A = 2 fN1 | B = 2 fN2 | C = 2 fN1
struct ProofWords {
  size_t fN1, fN2;
  explicit ProofWords(int curve) : fN1((size_t)msm_vtbl(curve, 1)->fN), fN2((size_t)msm_vtbl(curve, 2)->fN) {
    ZKP_REQUIRE(fN1 <= MAX_FN1 && fN2 <= MAX_FN2, ZKP_ERR_UNSUPPORTED_CURVE);
  }
  size_t affine() const { return 4 * fN1 + 2 * fN2; }
  int b_off() const { return (int)(2 * fN1); }
  int c_off() const { return (int)(2 * fN1 + 2 * fN2); }
};
constexpr size_t MAX_PROOF_WORDS = 4 * MAX_FN1 + 2 * MAX_FN2;
static_assert(MAX_PROOF_WORDS <= ASM_OUT_STEP, "an affine proof fits its slot of a fused group's device proofs");

// The lane's device proof buffer (PerLane::proof) for a group of G proofs: G x [r, s] | G x ASM_OUT_STEP proof words | G x flags
struct LaneProofBuf {
  static constexpr size_t WORDS = 1024;        // reserved per proof
  uint32_t *rs, *proof, *flags;
  LaneProofBuf(DevBuf& b, int G) : rs(b.as<uint32_t>(WORDS * G)), proof(rs + RS_STEP * G), flags(proof + ASM_OUT_STEP * G) {}
};
static_assert(RS_STEP + ASM_OUT_STEP + FLAG_STEP <= LaneProofBuf::WORDS, "[r, s], proof and flags fit what a proof reserves");

// The pinned landing zone of proof g of the lane's group (zkp_lane::host_proof holds MAX_FUSE of them).  Device tail: the affine
// proof at 0, its three flags at FLAGS.  Host tail: the points A | B | C as XYZZ, which prove_finish makes affine.
struct HostProofZone {
  static constexpr size_t FLAGS = 256;
  uint32_t *base, *a, *b, *c, *flags;
  HostProofZone(const zkp_lane* lane, int g, const ProofWords& w)
      : base(lane->host_proof + (size_t)g * zkp_lane::HOST_PROOF_WORDS), a(base), b(a + 4 * w.fN1), c(b + 4 * w.fN2), flags(base + FLAGS) {}
};
static_assert(MAX_PROOF_WORDS <= HostProofZone::FLAGS, "the affine proof ends in front of its flags");
static_assert(HostProofZone::FLAGS + 3 <= zkp_lane::HOST_PROOF_WORDS, "the flags lie inside the landing zone");
static_assert(8 * MAX_FN1 + 4 * MAX_FN2 <= zkp_lane::HOST_PROOF_WORDS, "three XYZZ points fit the landing zone");

// ctx->msm_misc as the two assembly entry points carve it: in_words of input | [r, s] | 6 result slots | the proof | its flags
struct AssembleBuf {
  static constexpr size_t PROOF_WORDS = 240, TAIL_WORDS = 256 + 16;      // the proof; proof + flags as reserved
  uint32_t *in, *rs;
  char* res;
  uint32_t *proof, *flags;
  AssembleBuf(zkp_ctx* ctx, size_t slot, size_t in_words) {
    in = ctx->msm_misc.as<uint32_t>(in_words + RS_STEP + 6 * slot / 4 + TAIL_WORDS);
    rs = in + in_words;
    res = reinterpret_cast<char*>(rs + RS_STEP);
    proof = reinterpret_cast<uint32_t*>(res + 6 * slot);
    flags = proof + PROOF_WORDS;
  }
  void upload_rs(hipStream_t st, const uint64_t* r, const uint64_t* s) const {
    ZKP_HIP(hipMemcpyAsync(rs, r, 32, hipMemcpyHostToDevice, st));
    ZKP_HIP(hipMemcpyAsync(rs + 8, s, 32, hipMemcpyHostToDevice, st));
  }
};
static_assert(MAX_PROOF_WORDS <= AssembleBuf::PROOF_WORDS && AssembleBuf::PROOF_WORDS + FLAG_STEP <= AssembleBuf::TAIL_WORDS,
              "proof and flags fit the tail of the carve-up");

// ---- the steps of a proof on one lane that ProofRun and the multi-device prover's legs share (groth16_pk.hpp)
// One proof's z, r, s into its S vector (nz + 4 scalars) and its [r, s] pair.  The copies and the tails are two calls because a
// captured graph holds the launch but not the copies.
void proof_copy_inputs(hipStream_t st, const zkp_groth16_pk* pk, const uint64_t* z, bool z_on_device, const uint64_t* r,
                       const uint64_t* s, uint32_t* S, uint32_t* rs) {
  ZKP_HIP(hipMemcpyAsync(S, z, pk->nz * 32, z_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  ZKP_HIP(hipMemcpyAsync(rs, r, 32, hipMemcpyHostToDevice, st));
  ZKP_HIP(hipMemcpyAsync(rs + 8, s, 32, hipMemcpyHostToDevice, st));
}
// the tails [1, r, s, -r*s] of the G consecutive S vectors of a group, one launch
void proof_scalar_tails(hipStream_t st, const zkp_groth16_pk* pk, uint32_t* S, const uint32_t* rs, int G) {
  with_fr(pk->curve, [&](auto P) {
    hipLaunchKernelGGL(scalar_tail_kernel<decltype(P)>, dim3(G), dim3(64), 0, st, S + pk->nz * 8, rs, (pk->nz + 4) * 8);
  });
}
// The request of query idx (0..4: A, B1, B2, H, L) over this key's slice of it: scalars = the witness map's output for H, S for the
// others; the sum goes to slot idx of res.  Workspace, sort sharing and the rest stay with the caller.
MsmJob proof_query_job(const zkp_groth16_pk* pk, int idx, const uint32_t* scalars, char* res, size_t slot) {
  const uint64_t handles[5] = {pk->hA, pk->hB1, pk->hB2, pk->hH, pk->hL};
  MsmJob m;
  m.handle = handles[idx];
  m.scalars_dev = reinterpret_cast<const uint64_t*>(scalars) + 4 * pk->q_lo[idx];
  m.n = pk->q_n[idx];
  m.montgomery = true;
  m.out_dev_xyzz = res + idx * slot;
  return m;
}
// the lane's workspace streams wait for what its main stream holds so far (S is complete) / the main stream waits for them
void lane_fork(zkp_lane* lane) {
  ZKP_HIP(hipEventRecord(lane->ev_fork, lane->stream));
  for (int w = 1; w < zkp_ctx::N_WS; w++) ZKP_HIP(hipStreamWaitEvent(lane->ws[w].stream, lane->ev_fork, 0));
}
void lane_join(zkp_lane* lane) {
  for (int w = 1; w < zkp_ctx::N_WS; w++) {
    ZKP_HIP(hipEventRecord(lane->ws[w].done, lane->ws[w].stream));
    ZKP_HIP(hipStreamWaitEvent(lane->stream, lane->ws[w].done, 0));
  }
}

// One proof, or one fused group of proofs, to enqueue on the current lane (ctx->cur); filled by field assignment.
// G > 1: a FUSED GROUP of G proofs over the same key in the kernel chain of one.  The
// inputs lie in group-wide buffers (S: G vectors of nz + 4 scalars; [r, s] pairs RS_STEP words apart), one scalar_tail launch covers
// the group, every MSM runs as ONE MSM over G scalar vectors (msm.hip `sets`: window tables, sort passes, task schedule, accumulate
// and reduction launches shared), the results fill G x 6 slots and every assembly kernel runs one workgroup per proof.  The
// witness map runs once per proof: the group's a and b vectors through one batched transform per kind (ntt_run_batch) measured
// the same (profiles/proof_fusion_bench.txt).  Only with the default stream plan of a pipelined batch.
struct ProofJob {
  const uint64_t* const* z = nullptr;          // G assignments, nz Fr (Montgomery) each
  bool z_on_device = false;
  const uint64_t *r = nullptr, *s = nullptr;   // proof g: r + 4 g, s + 4 g (host)
  int G = 1;
  // != nullptr (base-sharded key): no assembly; the 5 XYZZ sums of this rank's slices (A | B1 | B2 | H | L, G2-sized slots) are
  // left there (device) for the all-gather
  char* partial_out = nullptr;
};

// The four events of a profiled proof and the zkp_groth16_timing they fill.  Every member but add_msm is a no-op unless the
// context profiles.
struct PhaseTimer {
  zkp_ctx* const ctx;
  hipStream_t const st;
  const bool on;
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};      // phase begin, phase end, proof begin, proof end
  zkp_groth16_timing tm{};
  PhaseTimer(zkp_ctx* ctx, hipStream_t st) : ctx(ctx), st(st), on(ctx->profiling) {}
  PhaseTimer(const PhaseTimer&) = delete;
  ~PhaseTimer() {                                               // on every exit path (msm_run may throw)
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  void start() {
    if (!on) return;
    for (hipEvent_t& x : e) ZKP_HIP(hipEventCreate(&x));
    ZKP_HIP(hipEventRecord(e[2], st));
  }
  void tic() { if (on) ZKP_HIP(hipEventRecord(e[0], st)); }
  void toc(float* dst) {
    if (!on) return;
    ZKP_HIP(hipEventRecord(e[1], st));
    ZKP_HIP(hipEventSynchronize(e[1]));
    ZKP_HIP(hipEventElapsedTime(dst, e[0], e[1]));
  }
  // one MSM over n scalars: milliseconds of its accumulate kernel and of its scalar scan (0 where not measured), entries it sorted
  void add_msm(int idx, size_t n, float ms, float ms_scan, uint64_t entries) {
    tm.ms_msm_accumulate += ms;
    tm.msm_points += entries;
    tm.ms_msm_acc[idx] = ms;
    tm.msm_entries[idx] = entries;
    if (ms_scan > 0.f) {                     // algorithmic bytes of the scalar scan: scalars read by both passes + one 8-B word per entry
      tm.ms_msm_scan += ms_scan;
      tm.msm_scan_bytes += 2 * 32 * (uint64_t)n + 8 * entries;
      tm.msm_scan_launches += 1;
    }
    tm.msm_accumulate_launches += 1;
  }
  void finish() {
    if (!on) return;
    ZKP_HIP(hipEventRecord(e[3], st));
    ZKP_HIP(hipStreamSynchronize(st));
    ZKP_HIP(hipEventElapsedTime(&tm.ms_total, e[2], e[3]));
    ctx->last_timing = tm;
  }
};

// One ProofJob on the current lane (ctx->cur), phase by phase in launch order: everything is asynchronous up to and including the
// read-back of the 3 proof points into the lane's pinned host buffer; prove_finish() synchronises the lane and hands them out.
// Schedule.  profiling: everything on the main stream, one MSM at a time, with per-phase events (plan_serial).
// otherwise: the main stream (witness_map -> H) and the three workspace streams of the lane, forked after the scalar tail and joined
// before assembly (plan_round2, or plan_round1 with ZKP_LATENCY_PLAN=0).
// ZKP_SINGLE_STREAM=1: one stream per proof (no fan-out inside a proof); concurrency then comes from the lanes only
struct ProofRun {
  zkp_ctx* const ctx;
  zkp_groth16_pk* const pk;
  const ProofJob& job;
  zkp_lane* const lane;
  hipStream_t const st;
  const zkp_tune& tune;
  const MsmVtbl *const v1, *const v2;
  const ProofWords pw;
  const int G;
  const size_t slot;                   // uniform (G2-sized) result slot; proof g: slots 6 g .. 6 g + 5 (A, B1, B2, H, L, then T / C)
  const size_t s_stride, h_stride;     // scalars between the S / the h vectors of two proofs of a group
  const bool fan;                      // the proof fans out over the lane's workspace streams
  // zkp_ctx_config.host_affine = ZKP_OFF / ZKP_HOST_AFFINE=0: into_affine of the proof points on the device (rounds 1-3) instead of the host
  const bool host_tail;
  uint32_t* const S;
  const LaneProofBuf buf;
  char* const res;
  PhaseTimer timer;
  // what a phase leaves for the phases behind it
  uint32_t* h = nullptr;               // the witness map's output of proof 0 (proof g: h_stride scalars behind proof g - 1)
  bool l_done = false, g2_done = false, part1_done = false;     // the plan has run the L MSM / proof.b's into_affine / assembly part 1
  bool chained = false;                // L's buckets stay in workspace 1 for H to reduce with its own

  static const ProofJob& checked(zkp_ctx* ctx, const zkp_groth16_pk* pk, const ProofJob& job) {
    ZKP_REQUIRE((pk->shard_world > 0) == (job.partial_out != nullptr), ZKP_ERR_BAD_ARG);
    ZKP_REQUIRE(pk->hA != 0, ZKP_ERR_BAD_ARG);             // matrices-only key: use the sharded path
    ZKP_REQUIRE(job.G >= 1 && job.G <= zkp_lane::MAX_FUSE, ZKP_ERR_BAD_ARG);
    const bool default_plan = !ctx->profiling && !ctx->tune.single_stream && ctx->tune.latency_plan != 0;
    ZKP_REQUIRE(job.G == 1 || (job.z && !job.partial_out && default_plan), ZKP_ERR_BAD_ARG);
    return job;
  }
  ProofRun(zkp_ctx* ctx, zkp_groth16_pk* pk, const ProofJob& j)
      : ctx(ctx), pk(pk), job(checked(ctx, pk, j)), lane(ctx->cur), st(lane->stream), tune(ctx->tune), v1(msm_vtbl(pk->curve, 1)),
        v2(msm_vtbl(pk->curve, 2)), pw(pk->curve), G(job.G), slot(v2->xyzz_bytes), s_stride(pk->nz + 4), h_stride(3 * pk->N),
        fan(!ctx->profiling && !tune.single_stream), host_tail(ctx->cfg.host_affine && !job.partial_out),
        S(pk->lane[ctx->cur_idx].S.as<uint32_t>(s_stride * 8 * G)), buf(pk->lane[ctx->cur_idx].proof, G),
        res(reinterpret_cast<char*>(pk->lane[ctx->cur_idx].results.get(6 * slot * G))), timer(ctx, st) {
    timer.start();
  }

  // z, r, s into the lane's buffers: all that runs in front of a graph launch
  void copy_inputs() {
    for (int g = 0; g < G; g++)
      proof_copy_inputs(st, pk, job.z[g], job.z_on_device, job.r + 4 * g, job.s + 4 * g, S + g * s_stride * 8, buf.rs + RS_STEP * g);
  }

  // everything behind the inputs: what a hipGraph captures
  void enqueue() {
    proof_scalar_tails(st, pk, S, buf.rs, G);
    ctx->tl_tag.clear();
    ctx->mark(st, "start");
    if (fan) lane_fork(lane);
    // The witness map heads the longest chain of a proof (witness map -> H MSM -> assembly): its launches go out FIRST, before
    // the ~150 launches of the four other MSMs (0.5 ms of host time): single-proof latency 10.1 -> 9.65 ms (ZKP_WM_FIRST=0: after
    // them, as in round 1).  Making the other MSMs' accumulate kernels wait for it — a kernel timeline shows machine-filling
    // accumulates from three streams leaving its kernels few wave slots for milliseconds — was measured too: 10.3 ms, not kept.
    const bool wm_first = !fan || tune.wm_first;       // (the serial plan always maps first)
    if (wm_first) witness_maps();
    if (wm_first && fan) ctx->mark(st, "wm");
    // (Round 4, measured with ZKP_TIMELINE=1 and removed again: holding the accumulate kernels of A / B1 / B2 / L until the witness map
    //  is done — the map ends at 5.4 ms of an 8.2 ms proof when they start at 0.9 ms — and giving L a workspace of its own so that its
    //  accumulate need not wait for A's reduction chain: 8.6-8.8 / 8.6-8.9 / 9.3-9.6 ms (gate / workspace / both) against 8.0-8.4.  The
    //  machine-filling accumulates only change places; what ends last is still one accumulate + its reduction.  A third plan — main: map ->
    //  H (sorted, accumulated, reduction deferred) -> L on top of H's buckets; B2 at once; A / B1 accumulates held until H is sorted —
    //  proved correct and ran 9.2-9.7 ms.  profiles/r04_latency_experiments.txt.)
    if (!fan) plan_serial();
    else if (tune.latency_plan != 0) plan_round2();
    else plan_round1();
    if (!wm_first) witness_maps();
    // chained: on top of L's buckets (workspace 1): result slot 3 = h_acc + l', slot 4 = identity
    msm(3, 0, -1, -1, false, chained ? 1 : -1);        // prover.rs:186-187 (min(len) truncation in q_n)
    if (!l_done) msm(4, 0);                            // prover.rs:189-190
    if (fan) lane_join(lane);
    if (job.partial_out) {
      emit_partials();
    } else {
      assemble();
      read_back();
    }
    timer.finish();
  }

  // one witness map per proof on the main stream, each in its own abc region of the lane
  void witness_maps() {
    timer.tic();
    for (int g = 0; g < G; g++) {
      uint32_t* hg = witness_map_dev(ctx, pk, S + g * s_stride * 8, !pk->h_lagrange, g, G);
      if (g == 0) h = hg;
      ZKP_REQUIRE(hg == h + (size_t)g * h_stride * 8, ZKP_ERR_BAD_ARG);     // h sits at the same place in every region
    }
    timer.toc(&timer.tm.ms_witness_map);
  }

  // MSM idx (0..4: A, B1, B2, H, L) into result slot idx, on workspace ws of the lane and its stream (0: the main stream).
  // sort_src / l1_src: the workspace whose bucket sort / level-1 pass it reuses; defer / acc_into: the L -> H bucket chain (MsmJob)
  void msm(int idx, int ws, int sort_src = -1, int l1_src = -1, bool defer = false, int acc_into = -1) {
    static const char* const names[5] = {"A", "B1", "B2", "H", "L"};
    const bool on_h = idx == 3;                          // H runs over the witness map's output, the others over slices of S
    float ms = 0.f, ms_scan = 0.f;
    uint64_t entries = 0;
    ctx->tl_tag = names[idx];
    timer.tic();
#ifdef ZKP_ABLATION   // timing ablation builds only (ZKP_BUILD_DEFS=-DZKP_ABLATION -> variants/<tag>/): WRONG proofs, never in the shipped library
    ctx->dbg_skip_k8 = ((tune.debug_skip_k8_mask >> idx) & 1) && ctx->batch_mode;
#endif
    MsmJob m = proof_query_job(pk, idx, on_h ? h : S, res, slot);
    m.ms_accumulate = timer.on ? &ms : nullptr;
    m.ms_scan = timer.on ? &ms_scan : nullptr;
    m.n_entries = &entries;
    m.ws = ws;
    m.sort_src = sort_src;
    m.l1_src = l1_src;
    m.sets = G;
    m.set_stride = on_h ? h_stride : s_stride;
    m.out_stride = 6 * slot;
    m.defer_reduce = defer;
    m.acc_into = acc_into;
    msm_run(ctx, m);
    ctx->dbg_skip_k8 = false;
    timer.toc(&timer.tm.ms_msm[idx]);
    timer.add_msm(idx, m.n, ms, ms_scan, entries);
  }

  // Stream plan (round 2; default for single proofs AND the pipelined batch — measured 113.6 vs 111.2 proofs/s and 11.0 vs
  // 11.9 ms single-proof latency against the round-1 plan below, which ZKP_LATENCY_PLAN=0 restores):
  //   ws2: B2 | ws1: A -> L | ws3: B1 (B2's sort), then s*g_a + r*g1_b as soon as A exists | main: witness_map -> H
  // (A is enqueued first: with a shared level-1 pass B2's stream waits on an event that A's stream must have recorded)
  void plan_round2() {
    const int l1 = pk->share_l1 ? 1 : -1;
    const bool b_l1 = pk->share_l1 && pk->b_in_l1;
    if (!b_l1) msm(2, 2);
    msm(0, 1);
    ZKP_HIP(hipEventRecord(lane->ev_a, lane->ws[1].stream));
    if (b_l1) msm(2, 2, -1, l1);
    // proof.b needs B2 only: its into_affine runs on B2's stream as soon as the MSM is done instead of in the tail of the proof
    if (!job.partial_out && tune.g2_early && !host_tail) {
      v2->assemble_g2(lane->ws[2].stream, res, slot, buf.proof, buf.flags, pw.b_off(), G);
      g2_done = true;
    }
    msm(1, 3, pk->share_b_sort ? 2 : -1);
    chained = pk->chain_lh;
    msm(4, 1, pk->share_al_sort ? 1 : -1, l1, chained);   // A's sort / level-1 pass, still in this workspace
    l_done = true;
    if (!job.partial_out) {
      ZKP_HIP(hipStreamWaitEvent(lane->ws[3].stream, lane->ev_a, 0));
      v1->assemble_g1_part1(lane->ws[3].stream, res, slot, buf.rs, host_tail ? nullptr : buf.proof, buf.flags, G);
      part1_done = true;
      ctx->tl_tag.clear();
      ctx->mark(lane->ws[3].stream, "part1");
    }
  }

  // Stream plan of round 1 (longest chain first): ws2: B2 | ws1: A -> B1 | main: witness_map -> H | ws3: L, then part 1 after A, B1
  // (4 lanes x 4 streams = 16 streams).  ZKP_L_OWN_STREAM=0: L behind H on the main stream.
  void plan_round1() {
    msm(2, 2);                                         // prover.rs:182-184
    msm(0, 1);                                         // prover.rs:164-167
    msm(1, 1, pk->share_b_sort ? 2 : -1);              // prover.rs:170-177 (B2's bucket sort reused)
    // (A's sort is reused only when B1 does not re-sort on the same workspace in the meantime, i.e. when B1 takes B2's sort)
    if (tune.l_own_stream) {
      msm(4, 3, pk->share_al_sort && pk->share_b_sort ? 1 : -1);     // prover.rs:189-190
      l_done = true;
    }
    ZKP_HIP(hipEventRecord(lane->ev_b1, lane->ws[1].stream));
    // the two dynamic scalar multiplications (s*g_a, r*g1_b) are a ~2 ms single-lane chain each: start them as soon as
    // A and B1 exist so they hide under the remaining MSMs
    if (!job.partial_out) {
      ZKP_HIP(hipStreamWaitEvent(lane->ws[3].stream, lane->ev_b1, 0));
      v1->assemble_g1_part1(lane->ws[3].stream, res, slot, buf.rs, host_tail ? nullptr : buf.proof, buf.flags, G);
      part1_done = true;
    }
  }

  // profiling or ZKP_SINGLE_STREAM=1: the z-MSMs one after the other on the main stream, behind the witness map; H, L and both
  // parts of the assembly follow there
  void plan_serial() {
    msm(0, 0);
    msm(1, 0);
    msm(2, 0);
  }

  void emit_partials() {
    ZKP_HIP(hipMemcpyAsync(job.partial_out, res, 5 * slot, hipMemcpyDeviceToDevice, st));
    ZKP_HIP(hipGetLastError());
  }

  // what the plan has left of the assembly, on the main stream
  void assemble() {
    uint32_t* out = host_tail ? nullptr : buf.proof;     // host tail: the points stay XYZZ in their result slots
    timer.tic();
    if (!part1_done) v1->assemble_g1_part1(st, res, slot, buf.rs, out, buf.flags, G);
    v1->assemble_g1_part2(st, res, slot, out, buf.flags, pw.c_off(), G);
    if (!g2_done && !host_tail) v2->assemble_g2(st, res, slot, buf.proof, buf.flags, pw.b_off(), G);
    ZKP_HIP(hipGetLastError());
    timer.toc(&timer.tm.ms_assemble);
  }

  // the group's proofs into the lane's pinned landing zones; the lane is busy until prove_finish
  void read_back() {
    for (int g = 0; g < G; g++) {
      const HostProofZone hz(lane, g, pw);
      const char* rg = res + (size_t)g * 6 * slot;
      if (host_tail) {
        // the three proof points go back as XYZZ (A = slot 0, B = slot 2, C = slot 5); prove_finish makes them affine on the host
        // with one inversion (host_field.hpp) — three single-lane Fermat chains (0.25-0.32 ms each) leave the tail of the proof
        ZKP_HIP(hipMemcpyAsync(hz.a, rg, 16 * pw.fN1, hipMemcpyDeviceToHost, st));
        ZKP_HIP(hipMemcpyAsync(hz.b, rg + 2 * slot, 16 * pw.fN2, hipMemcpyDeviceToHost, st));
        ZKP_HIP(hipMemcpyAsync(hz.c, rg + 5 * slot, 16 * pw.fN1, hipMemcpyDeviceToHost, st));
      } else {
        ZKP_HIP(hipMemcpyAsync(hz.base, buf.proof + (size_t)g * ASM_OUT_STEP, pw.affine() * 4, hipMemcpyDeviceToHost, st));
        ZKP_HIP(hipMemcpyAsync(hz.flags, buf.flags + FLAG_STEP * g, 12, hipMemcpyDeviceToHost, st));
      }
    }
    ctx->tl_tag.clear();
    ctx->mark(st, "copied");
    lane->host_tail = host_tail;
    lane->busy = true;
    lane->group = G;
  }
};

static void prove_enqueue_eager(zkp_ctx* ctx, zkp_groth16_pk* pk, const ProofJob& job) {
  ProofRun run(ctx, pk, job);
  run.copy_inputs();
  run.enqueue();
}

// every device pointer a captured proof embeds: if any scratch buffer was reallocated since the capture (another, larger
// key used the lane), the graph is stale
static std::vector<const void*> lane_signature(zkp_ctx* ctx, zkp_groth16_pk* pk) {
  std::vector<const void*> sig;
  zkp_lane* L = ctx->cur;
  zkp_groth16_pk::PerLane& PL = pk->lane[ctx->cur_idx];
  for (DevBuf* b : {&PL.abc, &PL.S, &PL.results, &PL.proof, &L->ntt_scratch}) sig.push_back(b->p);
  for (int w = 0; w < zkp_lane::N_WS; w++) {
    MsmWorkspace& ws = L->ws[w];
    for (DevBuf* b : {&ws.keys, &ws.vals, &ws.keys2, &ws.vals2, &ws.sort_tmp, &ws.offsets, &ws.buckets, &ws.tmp, &ws.out,
                      &ws.sched, &ws.scan_tmp, &ws.scan_tmp2, &ws.partial, &ws.redo})
      sig.push_back(b->p);
  }
  sig.push_back(pk);
  return sig;
}

// One proof on the current lane.  With ZKP_GRAPH=1 the ~250 launches of a proof (4 streams, fork/join by events) are
// captured once per (key, lane) into a hipGraph and replayed; the inputs are copied in front of the graph launch.
// Lane states: 0 = never run, 1 = ran eagerly once (scratch allocated, signature recorded), 2 = captured.
static void prove_enqueue(zkp_ctx* ctx, zkp_groth16_pk* pk, const ProofJob& job) {
  if (!ctx->tune.graph || ctx->profiling || ctx->tune.single_stream) {
    prove_enqueue_eager(ctx, pk, job);
    return;
  }
  ZKP_REQUIRE(job.G == 1, ZKP_ERR_BAD_ARG);
  zkp_groth16_pk::PerLane& PL = pk->lane[ctx->cur_idx];
  hipStream_t st = ctx->cur->stream;
  const bool current = PL.graph_state != 0 && PL.sig == lane_signature(ctx, pk);
  if (PL.graph_state == 2 && !current) {                   // stale
    (void)hipGraphExecDestroy(PL.graph_exec);
    (void)hipGraphDestroy(PL.graph);
    PL.graph_exec = nullptr;
    PL.graph = nullptr;
    PL.graph_state = 0;
  }
  if (PL.graph_state == 0 || !current) {
    prove_enqueue_eager(ctx, pk, job);                     // allocates every scratch buffer
    PL.sig = lane_signature(ctx, pk);
    PL.graph_state = 1;
    return;
  }
  ProofRun run(ctx, pk, job);
  run.copy_inputs();
  if (PL.graph_state == 1) {
    ZKP_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    try {
      run.enqueue();
    } catch (...) {
      hipGraph_t g = nullptr;
      (void)hipStreamEndCapture(st, &g);
      if (g) (void)hipGraphDestroy(g);
      throw;
    }
    ZKP_HIP(hipStreamEndCapture(st, &PL.graph));
    ZKP_HIP(hipGraphInstantiate(&PL.graph_exec, PL.graph, nullptr, nullptr, 0));
    PL.graph_state = 2;
  }
  ZKP_HIP(hipGraphLaunch(PL.graph_exec, st));
  ctx->cur->busy = true;
}

static void prove_finish(zkp_ctx* ctx, zkp_groth16_pk* pk, uint64_t* proof_out, uint8_t* inf_out) {
  const ProofWords pw(pk->curve);
  ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));
  if (!ctx->tl.empty()) {
    std::string line = "[zkp timeline ms]";
    for (auto& m : ctx->tl) {
      float ms = 0.f;
      (void)hipEventSynchronize(m.second);
      (void)hipEventElapsedTime(&ms, ctx->tl[0].second, m.second);
      char buf[64];
      snprintf(buf, sizeof buf, " %s=%.2f", m.first.c_str(), ms);
      line += buf;
      if (&m != &ctx->tl[0]) (void)hipEventDestroy(m.second);
    }
    (void)hipEventDestroy(ctx->tl[0].second);
    ctx->tl.clear();
    fprintf(stderr, "%s\n", line.c_str());
  }
  // a fused group hands out its proofs one behind the other: they are consecutive proofs of the batch
  for (int g = 0; g < ctx->cur->group; g++) {
    const HostProofZone hz(ctx->cur, g, pw);
    uint32_t* po = reinterpret_cast<uint32_t*>(proof_out) + (size_t)g * pw.affine();
    if (ctx->cur->host_tail) {
      const hostf::HostField Fq = hostf::fq_field(pk->curve);
      hostf::groth16_points_into_affine(Fq, hz.a, hz.b, hz.c, po, inf_out + 3 * g);
    } else {
      memcpy(po, hz.base, pw.affine() * 4);
      for (int i = 0; i < 3; i++) inf_out[3 * g + i] = (uint8_t)hz.flags[i];
    }
  }
  ctx->cur->busy = false;
  ctx->cur->group = 1;
}

// the tail the two assembly entry points share: six result slots and [r, s] in `b` -> the proof and its flags on the host
static void assemble_and_fetch(zkp_ctx* ctx, int curve, const AssembleBuf& b, size_t slot, uint64_t* proof_out, uint8_t* inf_out) {
  const MsmVtbl* v1 = msm_vtbl(curve, 1);
  const MsmVtbl* v2 = msm_vtbl(curve, 2);
  const ProofWords pw(curve);
  hipStream_t st = ctx->cur->stream;
  v1->assemble_g1_part1(st, b.res, slot, b.rs, b.proof, b.flags, 1);
  v1->assemble_g1_part2(st, b.res, slot, b.proof, b.flags, pw.c_off(), 1);
  v2->assemble_g2(st, b.res, slot, b.proof, b.flags, pw.b_off(), 1);
  ZKP_HIP(hipGetLastError());
  uint32_t flags_host[FLAG_STEP] = {0, 0, 0, 0};
  ZKP_HIP(hipMemcpyAsync(proof_out, b.proof, pw.affine() * 4, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipMemcpyAsync(flags_host, b.flags, 12, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
  for (int i = 0; i < 3; i++) inf_out[i] = (uint8_t)flags_host[i];
}

void groth16_assemble(zkp_ctx* ctx, int curve, const uint64_t* sums, const uint64_t* r, const uint64_t* s,
                      uint64_t* proof_out, uint8_t* inf_out) {
  const MsmVtbl* v1 = msm_vtbl(curve, 1);
  const MsmVtbl* v2 = msm_vtbl(curve, 2);
  hipStream_t st = ctx->cur->stream;
  const size_t slot = v2->xyzz_bytes;
  const size_t j1 = 3 * (size_t)v1->fN, j2 = 3 * (size_t)v2->fN;          // words
  const size_t in_words = 4 * j1 + j2;
  const AssembleBuf b(ctx, slot, in_words);
  ZKP_HIP(hipMemcpyAsync(b.in, sums, in_words * 4, hipMemcpyHostToDevice, st));
  b.upload_rs(st, r, s);
  const size_t off[5] = {0, j1, 2 * j1, 2 * j1 + j2, 3 * j1 + j2};
  for (int i = 0; i < 5; i++) (i == 2 ? v2 : v1)->from_jacobian(st, b.in + off[i], b.res + i * slot);
  assemble_and_fetch(ctx, curve, b, slot, proof_out, inf_out);
}

size_t groth16_partials_bytes(int curve) { return 5 * msm_vtbl(curve, 2)->xyzz_bytes; }

// Base-sharded step, part 1 (this rank): witness map (replicated) + the five partial MSMs over this rank's slices.
// Everything stays in HBM: out_dev receives groth16_partials_bytes() bytes, complete when the call returns.
void groth16_prove_partials(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint64_t* z_dev, const uint64_t* r, const uint64_t* s,
                            void* out_dev) {
  ZKP_REQUIRE(pk->shard_world > 0, ZKP_ERR_BAD_ARG);
  ctx->cur = &ctx->lanes[0];
  ctx->cur_idx = 0;
  ProofJob job;
  job.z = &z_dev;
  job.z_on_device = true;
  job.r = r;
  job.s = s;
  job.partial_out = (char*)out_dev;
  prove_enqueue_eager(ctx, pk, job);
  ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));
}

// Base-sharded step, part 2 (every rank, after the all-gather): fold the `world` rank buffers slot by slot and assemble
// the proof (prover.rs:192-210).  gathered_dev: world x groth16_partials_bytes() bytes of device memory.
void groth16_fold_assemble(zkp_ctx* ctx, int curve, const void* gathered_dev, int world, const uint64_t* r,
                           const uint64_t* s, uint64_t* proof_out, uint8_t* inf_out) {
  ZKP_REQUIRE(world >= 1, ZKP_ERR_BAD_ARG);
  const MsmVtbl* v1 = msm_vtbl(curve, 1);
  const MsmVtbl* v2 = msm_vtbl(curve, 2);
  hipStream_t st = ctx->cur->stream;
  const size_t slot = v2->xyzz_bytes;
  const AssembleBuf b(ctx, slot, 0);
  b.upload_rs(st, r, s);
  v1->fold_slots(st, (const char*)gathered_dev, 5 * slot, world, slot, 0x1b, b.res);     // A, B1, H, L
  v2->fold_slots(st, (const char*)gathered_dev, 5 * slot, world, slot, 0x04, b.res);     // B2
  assemble_and_fetch(ctx, curve, b, slot, proof_out, inf_out);
}

void groth16_prove(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint64_t* z, bool z_on_device, const uint64_t* r,
                   const uint64_t* s, uint64_t* proof_out, uint8_t* inf_out) {
  ZKP_REQUIRE(pk->shard_world == 0, ZKP_ERR_BAD_ARG);     // a sharded key yields partial sums only
  ctx->cur = &ctx->lanes[0];
  ctx->cur_idx = 0;
  ctx->tl_on = ctx->tune.timeline && !ctx->profiling;
  ProofJob job;
  job.z = &z;
  job.z_on_device = z_on_device;
  job.r = r;
  job.s = s;
  prove_enqueue(ctx, pk, job);
  ctx->tl_on = false;
  prove_finish(ctx, pk, proof_out, inf_out);
}

// n proofs, software-pipelined over the lanes (8, or 4 above 2^22): group i+1 is enqueued before group i is awaited, so the
// latency-bound tails (bucket reduction, assembly) of one overlap the throughput-bound kernels of the next.
//
// Fused groups.  ZKP_PROOF_FUSE (compile time, 1 or 2) consecutive proofs share ONE kernel chain (ProofJob G > 1): the
// ~155 latency-bound launches of a proof (scans, task scheduling, pyramid tops, final sums, assembly) each use a sliver of the device
// but hold a hardware queue while they run, and they last about as long for two proofs as for one.  A group runs on one lane with
// that lane's four streams and the unchanged stream plan.  An odd remainder, profiling runs, ZKP_GRAPH=1, ZKP_SINGLE_STREAM=1,
// ZKP_LATENCY_PLAN=0, window-group keys and domains above 2^22 take the one-proof path.  -DZKP_PROOF_FUSE=1 is the code path
// without groups (A/B builds).
#ifndef ZKP_PROOF_FUSE
#define ZKP_PROOF_FUSE 2
#endif
static_assert(ZKP_PROOF_FUSE == 1 || ZKP_PROOF_FUSE == 2, "group size: 1 or 2; larger groups are not tested");
static_assert(ZKP_PROOF_FUSE <= zkp_lane::MAX_FUSE, "a lane's pinned landing zones hold MAX_FUSE proofs");
void groth16_prove_batch(zkp_ctx* ctx, zkp_groth16_pk* pk, size_t n, const uint64_t* const* z_dev, const uint64_t* r,
                         const uint64_t* s, uint64_t* proofs_out, uint8_t* inf_out, bool z_on_device) {
  const MsmVtbl* v1 = msm_vtbl(pk->curve, 1);
  const MsmVtbl* v2 = msm_vtbl(pk->curve, 2);
  const size_t pw64 = (4 * (size_t)v1->fN + 2 * (size_t)v2->fN) / 2;
  const bool prof = ctx->profiling;
  ZKP_REQUIRE(pk->shard_world == 0, ZKP_ERR_BAD_ARG);
  size_t pending[zkp_ctx::N_LANES] = {};
  // proofs in flight: 8 lanes x 4 streams = 2 streams per hardware queue with 16 queues, 8 with 4 (measured optimum at 2^20 and 16
  // queues: 4 lanes 102, 6 lanes 103, 8 lanes 108-110, 12 lanes 104 proofs/s); 4 above 2^22 where a lane's scratch is tens of GB.
  // ZKP_LANES overrides.  Consecutive proofs go to consecutive lanes, and which streams of lane l + 1 queue behind which of lane l is
  // settled when the context creates them (capi.hip, stream_place.hpp): with 1, 2 or 4 hardware queues the main stream of lane l + 1
  // shares its queue with ws1 of lane l, not with main of lane l, so the packets that open proof i + 1 do not wait behind the join,
  // part 2 and read-back that close proof i (a kernel trace shows nothing of proof i + 1 starting before proof i
  // has ended when all main streams share one queue).
  const int lanes_default = pk->log_n <= 22 ? 8 : 4;          // zkp_ctx_config.lanes / ZKP_LANES override it per context
  const int nl = std::max(1, std::min(ctx->cfg.lanes > 0 ? ctx->cfg.lanes : lanes_default, (int)zkp_ctx::N_LANES));
  auto select = [&](int l) {
    ctx->cur = &ctx->lanes[l];
    ctx->cur_idx = l;
  };
  struct BatchMode {                             // several proofs in flight: throughput tuning (msm.hip: segmented-sum chunk)
    zkp_ctx* c;
    ~BatchMode() { c->batch_mode = false; }
  } batch_mode{ctx};
  ctx->batch_mode = n > 1 && !prof;
  // proofs per kernel chain, when everything a fused group needs holds
  int fuse = 1;
  if (ZKP_PROOF_FUSE > 1 && ctx->batch_mode && !ctx->tune.graph && !ctx->tune.single_stream && ctx->tune.latency_plan != 0 &&
      pk->log_n <= 22) {
    fuse = ZKP_PROOF_FUSE;
    for (uint64_t hq : {pk->hA, pk->hB1, pk->hB2, pk->hH, pk->hL})
      if (!msm_sets_ok(ctx, hq, fuse)) fuse = 1;
  }
  auto enqueue = [&](size_t i, int G) {                      // proofs i .. i + G - 1 on the current lane
    ProofJob job;
    job.z = z_dev + i;
    job.z_on_device = z_on_device;
    job.r = r + 4 * i;
    job.s = s + 4 * i;
    job.G = G;
    prove_enqueue(ctx, pk, job);
  };
  try {
    // First pipelined batch of this key: a lane's scratch (bucket arrays, sort buffers, NTT scratch: GiBs at 2^22) is allocated
    // when a proof first runs on it, and hipMalloc synchronises the device.  A batch shorter than the lane count would leave
    // that to a later call's steady state (measured: a 12-proof batch after a 4-proof one ran at 11 instead of 19 proofs/s at
    // 2^22 BLS12-381), so the lanes this key has never used run the first proof once, results discarded.
    // A fused group needs larger scratch than one proof (and covers it), so a batch that will run groups warms with a group.
    if (ctx->batch_mode) {
      const int warm = (size_t)fuse <= n ? fuse : 1;
      std::vector<uint64_t> scratch_proof(pw64 * warm + 8);
      uint8_t scratch_inf[3 * zkp_lane::MAX_FUSE + 1];
      bool any = false;
      for (int l = 0; l < nl; l++) {
        if (pk->lane[l].warmed >= warm) continue;
        select(l);
        enqueue(0, warm);
        pk->lane[l].warmed = warm;
        any = true;
      }
      if (any)
        for (int l = 0; l < nl; l++) {
          select(l);
          if (ctx->cur->busy) prove_finish(ctx, pk, scratch_proof.data(), scratch_inf);
        }
    }
    size_t k = 0;                                            // groups (or single proofs) enqueued so far
    for (size_t i = 0; i < n; k++) {
      const int G = n - i >= (size_t)fuse ? fuse : 1;          // the remainder goes one proof at a time
      const int l = prof ? 0 : (int)(k % nl);
      select(l);
      if (ctx->cur->busy) prove_finish(ctx, pk, proofs_out + pending[l] * pw64, inf_out + pending[l] * 3);
      enqueue(i, G);
      if (G > 1) pk->fused_groups++;
      pending[l] = i;
      i += G;
    }
    for (int l = 0; l < zkp_ctx::N_LANES; l++) {
      select(l);
      if (ctx->cur->busy) prove_finish(ctx, pk, proofs_out + pending[l] * pw64, inf_out + pending[l] * 3);
    }
  } catch (...) {
    (void)hipDeviceSynchronize();
    for (auto& L : ctx->lanes) L.busy = false;
    select(0);
    throw;
  }
  select(0);
}

}  // namespace zkp
