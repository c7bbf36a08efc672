// RCCL all-gather between the devices of one process, resolved at run time (no link-time dependency: the host may already have
// loaded its own librccl).  Needs distinct devices.  The caller falls back to peer copies when it is unavailable.
//
// Watchdog (round 6).  The first multi-rank ncclCommInitAll and the first collective are the two places where a mis-configured
// node HANGS instead of failing (no IPC handles, a dead link, a peer that never joins), and a hung create_proof is worse than a
// slow one.  So the whole bring-up — dlopen, ncclCommInitAll, and a PROBE all-gather of 64 bytes per rank on throw-away streams
// and buffers — runs on a helper thread; the calling thread waits for it with a deadline (zkp_ctx_config.multi_exchange_timeout_ms
// / ZKP_MULTI_EXCHANGE_TIMEOUT_MS, default 30 s per stage).  The helper polls the probe's streams itself and, when they do not
// drain in time, aborts the communicators (ncclCommAbort makes RCCL's kernels exit).  Either way — probe failed, or the helper
// never came back — RCCL is marked unusable for the life of the process and rccl_watchdog_fired() says so.
// The caller's streams only ever see an all-gather on communicators whose probe completed.
// ZKP_DEBUG_RCCL_HANG=init | probe simulates the two hangs on any box (tests/test_gpu_multi.py).
#include "rccl_gather.hpp"

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <thread>

namespace zkp {

namespace {
struct RcclApi {
  struct Fns {
    void* lib = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommAbort)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  };
  // what the helper thread and the caller share; the caller may walk away from it (shared_ptr keeps it alive for a helper
  // that returns late)
  struct Attempt {
    std::mutex m;
    std::condition_variable cv;
    bool done = false, ok = false, abandoned = false;
    Fns f;
    RcclComms comms;
    std::string why;
  };
  Fns f;
  std::mutex mu;                    // the communicators are process-wide: one bring-up, and one group of collective calls, at a time
  // one set of communicators per device set, kept for the life of the process (a second root over other devices must not tear
  // down the communicators a first root is about to use)
  std::map<std::vector<int>, RcclComms> comms_of;
  bool unusable = false, watchdog_fired = false;
  std::string why;

  static void bring_up(std::shared_ptr<Attempt> at, std::vector<int> ids, int timeout_ms) {
    const char* hang = env_str("ZKP_DEBUG_RCCL_HANG");     // read live: this helper thread has no context
    Fns f;
    RcclComms comms(ids.size(), nullptr);
    std::string why;
    bool ok = false;
    do {
      for (const char* name : {"librccl.so", "librccl.so.1"})
        if ((f.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
      if (!f.lib) { why = "librccl.so not loadable"; break; }
      f.CommInitAll = reinterpret_cast<decltype(f.CommInitAll)>(dlsym(f.lib, "ncclCommInitAll"));
      f.CommDestroy = reinterpret_cast<decltype(f.CommDestroy)>(dlsym(f.lib, "ncclCommDestroy"));
      f.CommAbort = reinterpret_cast<decltype(f.CommAbort)>(dlsym(f.lib, "ncclCommAbort"));
      f.GroupStart = reinterpret_cast<decltype(f.GroupStart)>(dlsym(f.lib, "ncclGroupStart"));
      f.GroupEnd = reinterpret_cast<decltype(f.GroupEnd)>(dlsym(f.lib, "ncclGroupEnd"));
      f.AllGather = reinterpret_cast<decltype(f.AllGather)>(dlsym(f.lib, "ncclAllGather"));
      if (!f.CommInitAll || !f.CommDestroy || !f.GroupStart || !f.GroupEnd || !f.AllGather) { why = "librccl.so lacks a symbol"; break; }
      if (hang && !strcmp(hang, "init")) std::this_thread::sleep_for(std::chrono::hours(24));      // simulated: ncclCommInitAll never returns
      if (f.CommInitAll(comms.data(), (int)ids.size(), ids.data()) != 0) { why = "ncclCommInitAll failed"; comms.clear(); break; }
      // probe: one all-gather of 64 bytes per rank on streams and buffers nothing else uses
      const int n = (int)ids.size();
      std::vector<hipStream_t> st(n, nullptr);
      std::vector<void*> snd(n, nullptr), rcv(n, nullptr);
      bool issued = true;
      for (int k = 0; k < n && issued; k++)
        issued = hipSetDevice(ids[k]) == hipSuccess && hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking) == hipSuccess &&
                 hipMalloc(&snd[k], 64) == hipSuccess && hipMalloc(&rcv[k], 64 * (size_t)n) == hipSuccess &&
                 hipMemsetAsync(snd[k], k + 1, 64, st[k]) == hipSuccess;
      if (issued) {
        issued = f.GroupStart() == 0;
        for (int k = 0; k < n && issued; k++)
          issued = hipSetDevice(ids[k]) == hipSuccess && f.AllGather(snd[k], rcv[k], 64, /*ncclUint8*/ 1, comms[k], st[k]) == 0;
        issued = f.GroupEnd() == 0 && issued;
      }
      bool drained = false, right = true;
      if (issued) {
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms);
        while (!drained && std::chrono::steady_clock::now() < deadline) {
          drained = !(hang && !strcmp(hang, "probe"));                                     // simulated: the collective never completes
          for (int k = 0; k < n && drained; k++) drained = hipStreamQuery(st[k]) == hipSuccess;
          if (!drained) std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
        if (drained) {                                                                   // every rank holds byte k + 1 in slot k
          std::vector<uint8_t> got(64 * (size_t)n);
          for (int k = 0; k < n && right; k++) {
            right = hipSetDevice(ids[k]) == hipSuccess && hipMemcpy(got.data(), rcv[k], got.size(), hipMemcpyDeviceToHost) == hipSuccess;
            for (int j = 0; j < n && right; j++) right = got[64 * (size_t)j] == (uint8_t)(j + 1) && got[64 * (size_t)j + 63] == (uint8_t)(j + 1);
          }
        }
      }
      if (!issued || !drained || !right) {
        why = !issued ? "the probe all-gather could not be enqueued" : !drained ? "the probe all-gather did not complete within " + std::to_string(timeout_ms) + " ms"
                      : "the probe all-gather returned wrong bytes";
        for (void* c : comms)
          if (c) (void)(f.CommAbort ? f.CommAbort(c) : f.CommDestroy(c));
        comms.clear();
        if (!drained) break;                                                             // streams may still be wedged: leak the probe's resources
      }
      for (int k = 0; k < n; k++) {
        (void)hipSetDevice(ids[k]);
        if (st[k]) (void)hipStreamDestroy(st[k]);
        if (snd[k]) (void)hipFree(snd[k]);
        if (rcv[k]) (void)hipFree(rcv[k]);
      }
      ok = issued && drained && right;
    } while (false);
    std::lock_guard<std::mutex> lk(at->m);
    if (at->abandoned) {                                  // the caller gave up on this attempt: nobody will use these communicators
      for (void* c : comms)
        if (c && f.CommAbort) (void)f.CommAbort(c);
      return;
    }
    at->f = f;
    at->comms = ok ? comms : RcclComms();
    at->ok = ok;
    at->why = why;
    at->done = true;
    at->cv.notify_all();
  }

  // -> the communicators of this device set (rank order), or nullptr
  const RcclComms* ready(const std::vector<zkp_ctx*>& devs, int timeout_ms) {
    if (unusable) return nullptr;
    std::vector<int> ids;
    for (zkp_ctx* d : devs) ids.push_back(d->device);
    if (auto it = comms_of.find(ids); it != comms_of.end()) return &it->second;
    for (size_t i = 0; i < ids.size(); i++)
      for (size_t j = i + 1; j < ids.size(); j++)
        if (ids[i] == ids[j]) { why = "duplicate device ids"; return nullptr; }           // RCCL refuses duplicate devices (not sticky)
    timeout_ms = std::max(1, timeout_ms);
    auto at = std::make_shared<Attempt>();
    std::thread(bring_up, at, ids, timeout_ms).detach();
    std::unique_lock<std::mutex> lk(at->m);
    // two stages on the helper (communicator setup, probe), one deadline each, and a margin for the teardown
    const bool back = at->cv.wait_for(lk, std::chrono::milliseconds(2 * (long long)timeout_ms + 2000), [&] { return at->done; });
    if (!back) {
      at->abandoned = true;
      unusable = watchdog_fired = true;
      why = "RCCL bring-up (ncclCommInitAll + probe all-gather) did not return within " + std::to_string(2 * (long long)timeout_ms + 2000) + " ms";
      return nullptr;
    }
    f = at->f;
    if (!at->ok) {
      why = at->why;
      // a missing library is an ordinary "unavailable"; a failed init or probe is what the watchdog exists for
      unusable = true;
      watchdog_fired = f.lib != nullptr && at->why != "librccl.so lacks a symbol";
      return nullptr;
    }
    return &(comms_of[ids] = at->comms);
  }
};
RcclApi& rccl() {
  static RcclApi* api = new RcclApi();      // never destructed: communicators must not be torn down after the HIP runtime
  return *api;
}
}  // namespace

const RcclComms* rccl_comms_for(const std::vector<zkp_ctx*>& devs, int timeout_ms, std::string* why) {
  RcclApi& R = rccl();
  std::lock_guard<std::mutex> lk(R.mu);
  const RcclComms* comms = R.ready(devs, timeout_ms);
  if (!comms) *why = R.why;
  return comms;
}

void rccl_all_gather(const RcclComms& comms, const std::vector<zkp_ctx*>& devs, void* const* send, void* const* recv, size_t bytes) {
  RcclApi& R = rccl();
  // two roots over the same devices share these communicators (two prover threads of one process): their groups are enqueued one
  // after the other, in the same order on every rank
  std::lock_guard<std::mutex> lk(R.mu);
  ZKP_REQUIRE(R.f.GroupStart() == 0, ZKP_ERR_DEVICE);
  for (size_t k = 0; k < devs.size(); k++) {
    ZKP_HIP(hipSetDevice(devs[k]->device));
    ZKP_REQUIRE(R.f.AllGather(send[k], recv[k], bytes, /*ncclUint8*/ 1, comms[k], devs[k]->cur->stream) == 0, ZKP_ERR_DEVICE);
  }
  ZKP_REQUIRE(R.f.GroupEnd() == 0, ZKP_ERR_DEVICE);
}

bool rccl_watchdog_fired() {
  RcclApi& R = rccl();
  std::lock_guard<std::mutex> lk(R.mu);
  return R.watchdog_fired;
}

}  // namespace zkp
