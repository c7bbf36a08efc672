// Internal A/B switches of the kernels and schedules: ONE table.  Host only (no HIP): tests/c/tune_table.cpp compiles it alone.
//
// zkp_cfg (ctx.hpp) is the public, resolved configuration (zkp_ctx_config); zkp_tune holds what is NOT public: the losing arms of
// measured experiments, kept so that a measurement can be repeated, and a few debug levels.  Both are filled from the environment
// when a context is created (capi.hip zkp_ctx_create_ex) and never read again: two contexts of one process may differ, and no
// switch depends on which entry point ran first.  The measurements behind a default stay in the comment at its use site.
#pragma once
#include <cstdio>
#include <cstdlib>

namespace zkp {

// The environment is read here and nowhere else.  env_str also serves the reads that stay live on purpose: the ZKP_DEBUG_MSM
// prints at upload time (a test sets it on a context that already exists) and ZKP_DEBUG_RCCL_HANG (a helper thread, no context).
inline const char* env_str(const char* name) { return getenv(name); }
inline long long env_num(const char* name, long long dflt) { const char* e = env_str(name); return e ? atoll(e) : dflt; }
inline bool env_flag(const char* name, bool dflt) { const char* e = env_str(name); return e ? atoi(e) != 0 : dflt; }   // unset: dflt

constexpr int tune_pow2_ceil(int v) { int p = 1; while (p < v && p < (1 << 30)) p <<= 1; return p; }
constexpr int tune_pow2_floor(int v) { int p = 1; while (p <= v / 2) p <<= 1; return p; }
constexpr int tune_nt(int v) { return v >= 1024 ? 1024 : v >= 512 ? 512 : 256; }   // threads per workgroup: one of three instantiations
constexpr int TUNE_TASK_CAP_MAX = 128;     // == MSM_TASK_CAP, TUNE_PAIR_TOP_MAX == PAIR_TOP_MAX (msm_vtbl.hpp; static_assert in msm.hip)
constexpr int TUNE_PAIR_TOP_MAX = 2048;
constexpr int tune_task_cap(int v) { return v < 4 ? 0 : v > TUNE_TASK_CAP_MAX ? TUNE_TASK_CAP_MAX : v; }

// FLAG(field, "ENV", default, meaning)            unset: the default; set: on unless it reads as 0
// INT (field, "ENV", default, clamp(v), meaning)  unset: the default; set: clamp applied to v = atoi(value)
// MASK: an INT read with strtol(value, 0, 0) (hex allowed)
#define ZKP_TUNE_ROWS(FLAG, INT, MASK)                                                                                                    \
  /* ntt.hip */                                                                                                                           \
  INT (ntt_smax, "ZKP_NTT_SMAX", 9, v < 4 ? 4 : v > 10 ? 10 : v, "max radix bits per NTT pass, 4..10")                                    \
  FLAG(ntt_v2, "ZKP_NTT_V2", true, "unsaturated-limb NTT pass kernel; 0: the saturated one")                                              \
  FLAG(ntt_full, "ZKP_NTT_FULL", true, "full-size twiddle / coset tables; 0: two-level lookups")                                          \
  FLAG(ntt_fuse, "ZKP_NTT_FUSE", true, "witness-map transforms as fused pass chains; 0: separate transforms")                             \
  /* groth16_key.hip: key upload */                                                                                                       \
  FLAG(b_window, "ZKP_B_WINDOW", false, "B queries get window bits of their own, sized by their live bases")                              \
  INT (b_window_bits, "ZKP_B_WINDOW_BITS", -1, v < 0 ? 0 : v, "with ZKP_B_WINDOW: their window bits; unset: round(log2 live) - 2")        \
  INT (b_task_cap, "ZKP_B_TASK_CAP", -1, v < 0 ? 0 : v, "with ZKP_B_WINDOW: their entries per task; unset: 32")                           \
  FLAG(share_b_sort, "ZKP_SHARE_B_SORT", true, "B1 reuses B2's bucket sort")                                                              \
  FLAG(share_al_sort, "ZKP_SHARE_AL_SORT", true, "L reuses A's bucket sort when their identity patterns are close")                       \
  FLAG(share_l1, "ZKP_SHARE_L1", true, "one level-1 sort pass for A, B2 and L")                                                           \
  FLAG(chain_lh, "ZKP_CHAIN_LH", true, "H accumulates on top of L's buckets: one reduction for both")                                     \
  /* groth16.hip: one proof */                                                                                                            \
  FLAG(ntt_batch, "ZKP_NTT_BATCH", false, "witness map transforms a, b, c in one launch per pass")                                        \
  FLAG(single_stream, "ZKP_SINGLE_STREAM", false, "one stream per proof: no fan-out inside a proof, no graph")                            \
  FLAG(wm_first, "ZKP_WM_FIRST", true, "the witness map is enqueued before the four other MSMs")                                          \
  FLAG(l_own_stream, "ZKP_L_OWN_STREAM", true, "round-1 stream plan only: L on a stream of its own")                                      \
  INT (latency_plan, "ZKP_LATENCY_PLAN", -1, v, "0: the round-1 stream plan; unset or non-zero: the round-2 plan")                        \
  FLAG(g2_early, "ZKP_G2_EARLY", true, "proof.b made affine on B2's stream as soon as B2 is done")                                        \
  FLAG(graph, "ZKP_GRAPH", false, "capture a proof's launches per (key, lane) into a hipGraph and replay it")                             \
  FLAG(timeline, "ZKP_TIMELINE", false, "print phase offsets of every blocking proof to stderr")                                          \
  MASK(debug_skip_k8_mask, "ZKP_DEBUG_SKIP_K8_MASK", 0, v, "ablation builds only: bit i skips the reduction of MSM i (wrong proofs)")     \
  /* msm.hip: window plan of resident bases */                                                                                            \
  FLAG(msm_widen, "ZKP_MSM_WIDEN", true, "a lone MSM below 2^20 points takes wider windows; 0: round(log2 n)")                            \
  FLAG(msm_balanced, "ZKP_MSM_BALANCED", true, "windows of ceil / floor(T / W) bits; 0: equal widths and a thin top window")              \
  INT (table_k, "ZKP_TABLE_K", 0, v > 64 ? 64 : tune_pow2_ceil(v), "forced window-group size, a power of two <= 64; unset: by the table budget") \
  INT (task_cap, "ZKP_TASK_CAP", 0, tune_task_cap(v), "entries per accumulate task, 4..128; below 4 and unset: the caller's choice")      \
  INT (task_cap_g2, "ZKP_TASK_CAP_G2", -1, tune_task_cap(v), "the same for G2 bases; unset: ZKP_TASK_CAP")                                \
  /* msm.hip: one MSM */                                                                                                                  \
  INT (msm_chunk_first, "ZKP_MSM_CHUNK_FIRST", 2, v < 1 ? 1 : v, "first chunk of a chunked MSM = a chunk / this; 1: equal chunks")        \
  INT (sort_h1, "ZKP_SORT_H1", 0, v, "> 0: forced bits of the level-1 sort bins")                                                         \
  FLAG(sort_staged, "ZKP_SORT_STAGED", true, "level-1 scatter staged through LDS")                                                        \
  INT (sort_nt_hist, "ZKP_SORT_NT_HIST", 1024, tune_nt(v), "threads per workgroup of the level-1 histogram: 1024, 512 or 256")            \
  INT (sort_nt_scatter, "ZKP_SORT_NT_SCATTER", 512, tune_nt(v), "threads per workgroup of the staged scatter: 1024, 512 or 256")          \
  INT (task_nt, "ZKP_TASK_NT", 1024, tune_nt(v), "threads per workgroup of the task fill / order kernels: 1024, 512 or 256")              \
  FLAG(memset_buckets, "ZKP_MEMSET_BUCKETS", false, "zero the whole bucket array instead of the empty buckets only")                      \
  FLAG(debug_force_redo, "ZKP_DEBUG_FORCE_REDO", false, "tests: every eighth accumulate task goes through the exact redo kernel")         \
  INT (debug_msm, "ZKP_DEBUG_MSM", 0, v, "non-zero: check and print every MSM's task schedule (the upload-time prints read it live)")     \
  FLAG(pair_top_fuse_seg, "ZKP_PAIR_TOP_FUSE_SEG", true, "pyramid top and the segmented sums below it in one launch")                     \
  FLAG(pair_top, "ZKP_PAIR_TOP", true, "the top of the reduction pyramid in one launch")                                                  \
  INT (pair_top_max, "ZKP_PAIR_TOP_MAX", TUNE_PAIR_TOP_MAX, v < 2 ? TUNE_PAIR_TOP_MAX : tune_pow2_floor(v),                               \
       "entries of the level that one launch takes from, rounded down to a power of two")                                                 \
  INT (msm_var_c, "ZKP_MSM_VAR_C", 0, v == 4 || v == 8 || v == 16 ? v : 0, "window bits of a true variable-base MSM: 4, 8 or 16; else by size") \
  /* msm_acc.hip (through MsmVtbl::accumulate) */                                                                                         \
  INT (acc_lds_bytes, "ZKP_ACC_LDS_BYTES", 0, v, "dynamic LDS of the accumulate kernel: lowers its occupancy for experiments")            \
  INT (g2_acc_occ, "ZKP_G2_ACC_OCC", 2, v, "G2 accumulate compiled for 2 or 3 waves per SIMD; anything else: 1")                          \
  INT (g1_acc_occ, "ZKP_G1_ACC_OCC", 3, v, "saturated-limb G1 accumulate: 4 = compiled for four waves per SIMD")                          \
  INT (g1_acc_waves, "ZKP_G1_ACC_WAVES", 0, v, "unsaturated-limb G1 accumulate: 3 = compiled for three waves per SIMD")                   \
  /* marlin.hip */                                                                                                                        \
  FLAG(marlin_early, "ZKP_MARLIN_EARLY", true, "commitments of finished polynomials start before their round ends")                       \
  FLAG(marlin_early_fft, "ZKP_MARLIN_EARLY_FFT", false, "second-round transforms of z_a, z_b, z start in the first round")                \
  FLAG(marlin_host_affine, "ZKP_MARLIN_HOST_AFFINE", true, "a round's commitments made affine on the host")                               \
  FLAG(marlin_early_eval, "ZKP_MARLIN_EARLY_EVAL", false, "evaluations at beta run under the h_2 commitment")

struct zkp_tune {
#define ZKP_TUNE_FLAG(f, env, d, doc) bool f = d;
#define ZKP_TUNE_INT(f, env, d, clamp, doc) int f = d;
  ZKP_TUNE_ROWS(ZKP_TUNE_FLAG, ZKP_TUNE_INT, ZKP_TUNE_INT)
#undef ZKP_TUNE_FLAG
#undef ZKP_TUNE_INT
};

inline zkp_tune tune_from_env() {
  zkp_tune t;
#define ZKP_TUNE_FLAG(f, env, d, doc) t.f = env_flag(env, d);
#define ZKP_TUNE_INT(f, env, d, clamp, doc) if (const char* e = env_str(env)) { const int v = atoi(e); t.f = (clamp); }
#define ZKP_TUNE_MASK(f, env, d, clamp, doc) if (const char* e = env_str(env)) { const int v = (int)strtol(e, nullptr, 0); t.f = (clamp); }
  ZKP_TUNE_ROWS(ZKP_TUNE_FLAG, ZKP_TUNE_INT, ZKP_TUNE_MASK)
#undef ZKP_TUNE_FLAG
#undef ZKP_TUNE_INT
#undef ZKP_TUNE_MASK
  if (t.task_cap_g2 < 0) t.task_cap_g2 = t.task_cap;     // unset (a set value below 4 is 0: no override): G2 bases follow ZKP_TASK_CAP
  return t;
}

// NAME=value, one line per row, in table order
inline void tune_dump(const zkp_tune& t, FILE* out) {
#define ZKP_TUNE_ANY(f, env, ...) fprintf(out, "%s=%d\n", env, (int)t.f);
  ZKP_TUNE_ROWS(ZKP_TUNE_ANY, ZKP_TUNE_ANY, ZKP_TUNE_ANY)
#undef ZKP_TUNE_ANY
}

}  // namespace zkp
using zkp::zkp_tune;     // named like zkp_cfg, beside which it sits in zkp_ctx
