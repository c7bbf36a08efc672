// Single-process multi-GPU (BASELINE configs[4]): the caller of `create_proof` (prover.rs:124) is ONE
// process, so the library owns one context per device (zkp_ctx_create_multi) and the exchange step itself.
//   shard      every (extended) query is split by index over the devices (rank k keeps 1/n of the window tables); one proof
//              uses all devices: partial MSMs per device -> partial sums gathered on device 0 over xGMI (peer copies of
//              n x 1.25 KiB; optionally an RCCL all-gather) -> fold + assembly on device 0.  With >= 3 devices the witness map
//              is task-split: the three independent chains of r1cs_to_qap.rs:144-162 (A z / B z / C z -> ifft -> coset_fft) run
//              on devices 0 / 1 / 2, the b and c coset evaluations are gathered on device 0 (pointwise step + coset_ifft), and
//              every device receives its slice of h for its share of the H MSM.
//   replicate  full key on every device, independent proofs dealt round-robin, one host thread per device driving that
//              device's pipelined lanes (zkp_groth16_prove_batch semantics).
// Everything is enqueued from the calling thread with streams and cross-device events; device ids may repeat (several ranks
// on ONE GPU: the tests on a one-GPU box), peer copies then degenerate to device-to-device copies.
// Host code only: the kernels of a device's leg are those of the single-device prover, reached through groth16_pk.hpp.
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "groth16_pk.hpp"
#include "internal.hpp"
#include "msm_vtbl.hpp"
#include "rccl_gather.hpp"

struct zkp_groth16_pk_multi {
  int mode = 0, curve = 0;
  struct PerDevice {                        // one per device of the root context, rank order
    zkp_groth16_pk* pk = nullptr;
    hipEvent_t ev_chain = nullptr, ev_done = nullptr, ev_h_read = nullptr;
    void* partial = nullptr;                // 5 XYZZ slots
    void* gathered = nullptr;               // n x partials bytes: what the exchange fills (peer copies: device 0's only)
  };
  std::vector<PerDevice> dev;
  hipEvent_t ev_h = nullptr;
  // run-time choices of the sharded prover (zkp_groth16_multi_info): which exchange carried the last proof, and whether the
  // three chains of the witness map are split over devices 0..2 — measured on this key's own first proofs, not assumed
  int exchange = 0;                         // 0 = peer copies, 1 = RCCL all-gather, 2 = peer copies after the RCCL watchdog gave up
  bool exchange_fallback = false;
  int rccl_ranks = 0;
  int split_choice = -1;                    // -1 undecided, 0 replicated witness map, 1 three-way split
  int calls = 0;
  double ms_variant[2] = {0.0, 0.0};        // wall time of a proof with the replicated / split witness map (calls 3 and 4)
};

namespace zkp {

namespace {
void copy_between(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st) {
  if (!bytes) return;
  if (dst_dev == src_dev) ZKP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
  else ZKP_HIP(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st));
}

// One base-sharded proof over the devices of `root`, phase by phase in launch order.  Device k's leg runs on lane 0 of its context:
// the main stream (its part of the witness map -> H) and the lane's three workspace streams (the z-MSMs).  run() makes three passes
// over the devices — phase 1 of every device, the gather of the split witness map, phase 3 of every device — so that the witness
// maps and z-MSMs of all devices are out before any H MSM: that order is what lets the devices overlap.
struct MultiProofRun {
  zkp_ctx* const root;
  zkp_groth16_pk_multi* const M;
  const uint64_t* const* const z;           // z_on_device: one assignment per device, there; else one on the host
  const bool z_on_device;
  const uint64_t *const r, *const s;
  const int n;
  const size_t slot, pb;                    // bytes of a (G2-sized) result slot and of a device's five partial sums
  struct Leg {                              // device k's lane buffers, resolved by stage_inputs(k); h: where its H scalars lie
    uint32_t *S = nullptr, *abc = nullptr, *h = nullptr;
    char* res = nullptr;
  };
  std::vector<Leg> leg;
  bool split = false;                       // the witness map's a / b / c chains run on devices 0 / 1 / 2
  const RcclComms* rccl = nullptr;          // != nullptr: the partial sums travel by an RCCL all-gather on these
  int call = 0;
  std::chrono::steady_clock::time_point t_call;

  MultiProofRun(zkp_ctx* root, zkp_groth16_pk_multi* M, const uint64_t* const* z, bool z_on_device, const uint64_t* r, const uint64_t* s)
      : root(root), M(M), z(z), z_on_device(z_on_device), r(r), s(s), n((int)root->devs.size()),
        slot(msm_vtbl(M->curve, 2)->xyzz_bytes), pb(5 * slot), leg(n) {}

  void run(uint64_t* proof_out, uint8_t* inf_out) {
    choose_witness_variant();
    choose_exchange();
    for (int k = 0; k < n; k++) {           // phase 1
      stage_inputs(k);
      witness_part(k);
      z_msms(k);
    }
    if (split) gather_witness();            // phase 2
    for (int k = 0; k < n; k++) h_msm_and_partials(k);      // phase 3
    exchange();                             // phase 4
    fold_and_settle(proof_out, inf_out);
  }

  zkp_ctx* ctx(int k) const { return root->devs[k]; }
  zkp_groth16_pk* pk(int k) const { return M->dev[k].pk; }
  int nchain() const { return pk(0)->c_folded ? 2 : 3; }    // C folded into the L query: no c chain
  hipStream_t enter(int k) const {                          // device k current -> its main stream
    ZKP_HIP(hipSetDevice(ctx(k)->device));
    return ctx(k)->cur->stream;
  }

  // Witness map: replicated on every device, or its a / b / c chains on devices 0 / 1 / 2 with two N x 32-byte vectors shipped to
  // device 0 and the slices of h shipped back (n >= 3).  Which one is faster depends on the link (one xGMI hop vs. a PCIe switch)
  // and on the domain, so the key MEASURES it: proofs 1-2 warm both variants up, proofs 3-4 time them (wall clock of the whole
  // call, same witness), from proof 5 on the faster one runs.  The proof bytes do not depend on the choice.
  // ZKP_MULTI_WM_SPLIT=0 / 1 forces a variant.
  void choose_witness_variant() {
    const int split_env = root->cfg.multi_wm_split;               // zkp_ctx_config.multi_witness_split / ZKP_MULTI_WM_SPLIT
    call = M->calls++;
    if (n >= 3) {
      if (split_env >= 0) M->split_choice = split_env ? 1 : 0;
      if (M->split_choice >= 0) split = M->split_choice == 1;
      else split = (call & 1) == 1;                                   // calls 0, 2: replicated; 1, 3: split
    } else {
      M->split_choice = 0;
    }
    t_call = std::chrono::steady_clock::now();
  }

  // Exchange: RCCL all-gather (the exchange BASELINE.json names) whenever the devices are distinct and librccl loads; peer copies
  // otherwise, said once on stderr.  ZKP_MULTI_EXCHANGE=peer / rccl forces one.
  // ZKP_MULTI_EXCHANGE=rccl also takes the RCCL branch with ONE rank (a one-rank ncclCommInitAll + ncclAllGather is legal): the
  // hand-declared prototypes of rccl_gather.hip get executed on a one-GPU box (tests/test_gpu_multi.py) before any 8-GPU node sees them.
  void choose_exchange() {
    const int want = root->cfg.multi_exchange;                     // zkp_ctx_config.multi_exchange / ZKP_MULTI_EXCHANGE, per context
    if ((n > 1 && want != ZKP_EXCHANGE_PEER) || (n == 1 && want == ZKP_EXCHANGE_RCCL)) {
      std::string why;
      rccl = rccl_comms_for(root->devs, root->cfg.multi_exchange_timeout_ms, &why);
      const bool watchdog = !rccl && rccl_watchdog_fired();
      static std::atomic<bool> told{false};
      if (!rccl && !told.exchange(true))
        fprintf(stderr, "[zkp_accel] sharded prover: RCCL all-gather unavailable (%s)%s — the partial sums travel by peer copies\n",
                why.c_str(), watchdog ? " [watchdog: RCCL stays off for this process]" : "");
      if (watchdog) M->exchange_fallback = true;
    }
    M->exchange = rccl ? 1 : (M->exchange_fallback ? 2 : 0);
    M->rccl_ranks = rccl ? n : 0;
  }

  // phase 1 — every device: inputs, its part of the witness map, the four z-MSMs over its slices on the MSM streams
  void stage_inputs(int k) {
    zkp_ctx* c = ctx(k);
    zkp_groth16_pk* p = pk(k);
    ZKP_HIP(hipSetDevice(c->device));
    c->cur = &c->lanes[0];
    c->cur_idx = 0;
    zkp_groth16_pk::PerLane& PL = p->lane[0];
    Leg& L = leg[k];
    L.S = PL.S.as<uint32_t>((p->nz + 4) * 8);
    uint32_t* rs = PL.proof.as<uint32_t>(1024);
    L.res = reinterpret_cast<char*>(PL.results.get(6 * slot));
    proof_copy_inputs(c->cur->stream, p, z_on_device ? z[k] : z[0], z_on_device, r, s, L.S, rs);
    proof_scalar_tails(c->cur->stream, p, L.S, rs, 1);
    lane_fork(c->cur);
  }

  // the whole map, or with the split this device's chain (evaluate k, transform k) in region k of its abc
  void witness_part(int k) {
    zkp_ctx* c = ctx(k);
    zkp_groth16_pk* p = pk(k);
    Leg& L = leg[k];
    L.abc = p->lane[0].abc.as<uint32_t>(3 * p->N * 8);
    if (!split) {
      L.h = witness_map_dev(c, p, L.S, !p->h_lagrange);
    } else if (k < nchain()) {
      witness_eval(c, p, L.S, k, L.abc + (size_t)k * p->N * 8);
      witness_transform(c, p, L.abc + (size_t)k * p->N * 8);
      ZKP_HIP(hipGetLastError());
      ZKP_HIP(hipEventRecord(M->dev[k].ev_chain, c->cur->stream));
    }
  }

  // B2 | A -> L | B1 on workspaces 2 | 1 | 3 with the sort and level-1 sharing of the key, as ProofRun::plan_round2 orders them
  void z_msms(int k) {
    zkp_ctx* c = ctx(k);
    zkp_groth16_pk* p = pk(k);
    auto msm = [&](int idx, int ws, int sort_src, int l1_src) {
      MsmJob m = proof_query_job(p, idx, leg[k].S, leg[k].res, slot);
      m.ws = ws;
      m.sort_src = sort_src;
      m.l1_src = l1_src;
      msm_run(c, m);
    };
    const int l1 = p->share_l1 ? 1 : -1;
    const bool b_l1 = p->share_l1 && p->b_in_l1;
    if (!b_l1) msm(2, 2, -1, -1);
    msm(0, 1, -1, -1);
    if (b_l1) msm(2, 2, -1, l1);
    msm(1, 3, p->share_b_sort ? 2 : -1, -1);
    msm(4, 1, p->share_al_sort ? 1 : -1, l1);
  }

  // phase 2 (task-split witness map) — device 0 gathers b and c, finishes h, every device fetches its slice of h
  void gather_witness() {
    zkp_ctx* c0 = ctx(0);
    zkp_groth16_pk* p0 = pk(0);
    hipStream_t st0 = enter(0);
    for (int k = 1; k < nchain(); k++) {
      const size_t region = (size_t)k * p0->N * 8;
      ZKP_HIP(hipStreamWaitEvent(st0, M->dev[k].ev_chain, 0));
      copy_between(leg[0].abc + region, c0->device, leg[k].abc + region, ctx(k)->device, p0->N * 32, st0);
    }
    leg[0].h = witness_finish(c0, p0, leg[0].abc, !p0->h_lagrange);
    ZKP_HIP(hipEventRecord(M->ev_h, st0));
    for (int k = 1; k < n; k++) {
      zkp_groth16_pk* p = pk(k);
      hipStream_t st = enter(k);
      leg[k].h = leg[k].abc;                                     // region a of this device (its own chain, if any, is consumed)
      ZKP_HIP(hipStreamWaitEvent(st, M->ev_h, 0));
      if (k < nchain()) ZKP_HIP(hipStreamWaitEvent(st, M->dev[k].ev_chain, 0));
      copy_between(leg[k].h + p->q_lo[3] * 8, ctx(k)->device, leg[0].h + p->q_lo[3] * 8, c0->device, p->q_n[3] * 32, st);
      ZKP_HIP(hipEventRecord(M->dev[k].ev_h_read, st));
    }
  }

  // phase 3 — every device: H MSM over its slice of h, join, partial sums
  void h_msm_and_partials(int k) {
    hipStream_t st = enter(k);
    msm_run(ctx(k), proof_query_job(pk(k), 3, leg[k].h, leg[k].res, slot));
    lane_join(ctx(k)->cur);
    ZKP_HIP(hipMemcpyAsync(M->dev[k].partial, leg[k].res, pb, hipMemcpyDeviceToDevice, st));
    ZKP_HIP(hipEventRecord(M->dev[k].ev_done, st));
  }

  // phase 4 — exchange (n x 1.25 KiB for BN254: latency-bound on any topology): every device's partial sums into device 0's `gathered`
  void exchange() {
    if (rccl) {
      std::vector<void*> send(n), recv(n);
      for (int k = 0; k < n; k++) send[k] = M->dev[k].partial, recv[k] = M->dev[k].gathered;
      rccl_all_gather(*rccl, root->devs, send.data(), recv.data(), pb);
    }
    hipStream_t st0 = enter(0);
    if (!rccl)
      for (int k = 0; k < n; k++) {
        if (k) ZKP_HIP(hipStreamWaitEvent(st0, M->dev[k].ev_done, 0));
        copy_between((char*)M->dev[0].gathered + (size_t)k * pb, ctx(0)->device, M->dev[k].partial, ctx(k)->device, pb, st0);
      }
    if (split)                                     // h on device 0 must outlive the slice reads of the other devices
      for (int k = 1; k < n; k++) ZKP_HIP(hipStreamWaitEvent(st0, M->dev[k].ev_h_read, 0));
  }

  // fold + assembly on device 0; the split-timing bookkeeping of choose_witness_variant
  void fold_and_settle(uint64_t* proof_out, uint8_t* inf_out) {
    groth16_fold_assemble(ctx(0), M->curve, M->dev[0].gathered, n, r, s, proof_out, inf_out);        // synchronises device 0's stream
    for (int k = 1; k < n; k++) ZKP_HIP(hipStreamSynchronize(enter(k)));                            // the next call reuses every device's buffers
    enter(0);
    if (n >= 3 && M->split_choice < 0 && call >= 2) {
      M->ms_variant[split ? 1 : 0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count();
      if (call >= 3) M->split_choice = M->ms_variant[1] < M->ms_variant[0] ? 1 : 0;
    }
  }
};
}  // namespace

zkp_groth16_pk_multi* groth16_pk_upload_multi(zkp_ctx* root, const zkp_groth16_pk_desc* d, int mode) {
  ZKP_REQUIRE(!root->devs.empty() && (mode == 0 || mode == 1), ZKP_ERR_BAD_ARG);
  const int n = (int)root->devs.size();
  std::unique_ptr<zkp_groth16_pk_multi> M(new zkp_groth16_pk_multi());
  M->mode = mode;
  M->curve = d->curve;
  KeepLagrange keep_lagrange;                      // one transform of the H query serves every device (groth16_pk.hpp)
  try {
    for (int k = 0; k < n; k++) {
      zkp_ctx* ctx = root->devs[k];
      ZKP_HIP(hipSetDevice(ctx->device));
      M->dev.emplace_back();                       // filled in place: groth16_pk_multi_free releases whatever a failure leaves
      zkp_groth16_pk_multi::PerDevice& D = M->dev.back();
      D.pk = mode == 0 ? groth16_pk_upload(ctx, d, k, n) : groth16_pk_upload(ctx, d, 0, 0);
      for (hipEvent_t* e : {&D.ev_chain, &D.ev_done, &D.ev_h_read}) ZKP_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
      if (hipMalloc(&D.partial, groth16_partials_bytes(d->curve)) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
      if (hipMalloc(&D.gathered, (size_t)n * groth16_partials_bytes(d->curve)) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
    }
    ZKP_HIP(hipSetDevice(root->device));
    ZKP_HIP(hipEventCreateWithFlags(&M->ev_h, hipEventDisableTiming));
  } catch (...) {
    groth16_pk_multi_free(root, M.release());
    throw;
  }
  return M.release();
}

void groth16_pk_multi_free(zkp_ctx* root, zkp_groth16_pk_multi* M) {
  for (size_t k = 0; k < M->dev.size(); k++) {
    zkp_groth16_pk_multi::PerDevice& D = M->dev[k];
    (void)hipSetDevice(root->devs[k]->device);
    if (D.pk) groth16_pk_free(root->devs[k], D.pk);
    if (D.partial) (void)hipFree(D.partial);
    if (D.gathered) (void)hipFree(D.gathered);
    for (hipEvent_t e : {D.ev_chain, D.ev_done, D.ev_h_read})
      if (e) (void)hipEventDestroy(e);
  }
  if (M->ev_h) (void)hipEventDestroy(M->ev_h);
  (void)hipSetDevice(root->device);
  delete M;
}

// info[0] = exchange of the last proof (0 peer copies, 1 RCCL all-gather), [1] = RCCL ranks, [2] = witness map (0 replicated, 1 split
// over devices 0..2, 2 = still measuring), [3] / [4] = microseconds of the timed proof with the replicated / split map, [5] = devices
void groth16_multi_info(zkp_ctx* root, zkp_groth16_pk_multi* M, uint64_t info[6]) {
  info[0] = (uint64_t)M->exchange;
  info[1] = (uint64_t)M->rccl_ranks;
  info[2] = M->split_choice < 0 ? 2 : (uint64_t)M->split_choice;
  info[3] = (uint64_t)(M->ms_variant[0] * 1e3);
  info[4] = (uint64_t)(M->ms_variant[1] * 1e3);
  info[5] = (uint64_t)root->devs.size();
}

void groth16_prove_multi(zkp_ctx* root, zkp_groth16_pk_multi* M, const uint64_t* const* z, bool z_on_device,
                         const uint64_t* r, const uint64_t* s, uint64_t* proof_out, uint8_t* inf_out) {
  ZKP_REQUIRE(M->mode == 0 && M->dev.size() == root->devs.size() && !root->devs.empty(), ZKP_ERR_BAD_ARG);
  try {
    MultiProofRun(root, M, z, z_on_device, r, s).run(proof_out, inf_out);
  } catch (...) {
    for (zkp_ctx* c : root->devs) {
      (void)hipSetDevice(c->device);
      (void)hipDeviceSynchronize();
    }
    (void)hipSetDevice(root->device);
    throw;
  }
}

// Throughput mode on every device of the root context: proof i runs on device i % n (its witness pointer, when
// z_on_device, lives there); one host thread per device drives that device's lanes exactly as zkp_groth16_prove_batch does.
void groth16_prove_batch_multi(zkp_ctx* root, zkp_groth16_pk_multi* M, size_t count, const uint64_t* const* z,
                               bool z_on_device, const uint64_t* r, const uint64_t* s, uint64_t* proofs_out,
                               uint8_t* inf_out) {
  ZKP_REQUIRE(M->mode == 1 && M->dev.size() == root->devs.size() && !root->devs.empty(), ZKP_ERR_BAD_ARG);
  const int n = (int)root->devs.size();
  const MsmVtbl* v1 = msm_vtbl(M->curve, 1);
  const MsmVtbl* v2 = msm_vtbl(M->curve, 2);
  const size_t pw64 = (4 * (size_t)v1->fN + 2 * (size_t)v2->fN) / 2;
  std::vector<int32_t> status(n, ZKP_OK);
  std::vector<std::thread> th;
  for (int k = 0; k < n; k++) {
    th.emplace_back([&, k] {
      try {
        zkp_ctx* ctx = root->devs[k];
        ZKP_HIP(hipSetDevice(ctx->device));
        std::vector<const uint64_t*> zk;
        std::vector<uint64_t> rk, sk;
        for (size_t i = (size_t)k; i < count; i += (size_t)n) {
          zk.push_back(z[i]);
          rk.insert(rk.end(), r + 4 * i, r + 4 * i + 4);
          sk.insert(sk.end(), s + 4 * i, s + 4 * i + 4);
        }
        if (zk.empty()) return;
        std::vector<uint64_t> po(zk.size() * pw64);
        std::vector<uint8_t> io(zk.size() * 3);
        groth16_prove_batch(ctx, M->dev[k].pk, zk.size(), zk.data(), rk.data(), sk.data(), po.data(), io.data(), z_on_device);
        size_t j = 0;
        for (size_t i = (size_t)k; i < count; i += (size_t)n, j++) {
          memcpy(proofs_out + i * pw64, po.data() + j * pw64, pw64 * 8);
          memcpy(inf_out + i * 3, io.data() + j * 3, 3);
        }
      } catch (...) {
        HipError e{hipSuccess, nullptr, 0};
        status[k] = status_of_current_exception(&e);
        if (e.what) fprintf(stderr, "[zkp_accel] HIP error %s at line %d: %s (device rank %d)\n", hipGetErrorString(e.e), e.line, e.what, k);
      }
    });
  }
  for (auto& t : th) t.join();
  (void)hipSetDevice(root->device);
  for (int32_t st : status)
    if (st != ZKP_OK) throw StatusError{st};
}

}  // namespace zkp
