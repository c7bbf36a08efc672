// Geometry of the MSM bucket sort and of the task schedule (msm.hip K6 / K7): how many level-1 bins and tiles, what the kernels
// need of LDS, where the arrays of the schedule lie in one buffer.  Pure host arithmetic without HIP: tests/c/sort_plan.cpp includes
// this header alone and compares it with the integer model in tests/msm_plan_ref.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {

constexpr int SORT_H1_MAX = 13;        // level-1 bins <= 8192 (static LDS histogram, 32 KiB)
constexpr uint32_t SORT_BIN_TARGET = 16384;   // entries per level-1 bin the level-2 kernel stages in LDS
constexpr int SORT_L_MAX = 13;         // level-2 keys per bin <= 8192 (dynamic LDS)
// scalars per workgroup in the level-1 passes (8 per lane): larger tiles = smaller (bin x tile) count matrix and longer contiguous
// runs per bin in the scatter (512 -> 2048: +2 % proofs/s).  The default; larger MSMs use larger tiles (SortPlan::tile) to keep
// the tile count ~1200
constexpr int SORT_SCALARS = 2048;
#ifndef ZKP_SORT_STAGE_BYTES              // A/B builds (ZKP_BUILD_DEFS_msm): 28 KiB = five workgroups per CU instead of two
#define ZKP_SORT_STAGE_BYTES (56 * 1024)
#endif
constexpr uint32_t SORT_STAGE_BYTES = ZKP_SORT_STAGE_BYTES;   // LDS stage of the staged level-1 scatter (sort_scatter_staged_kernel)
constexpr uint32_t SORT_BIN_THREADS = 1024;
#ifndef ZKP_SORT_BIN_STAGE                      // A/B builds: 18432 (72 KiB) lets two workgroups share a CU
#define ZKP_SORT_BIN_STAGE 20480
#endif
constexpr uint32_t SORT_BIN_STAGE = ZKP_SORT_BIN_STAGE;      // values staged in LDS (80 KiB) so the output is written fully coalesced
constexpr int TM_WORDS = 512;          // words of the schedule's tmeta block (msm.hip TM_*)

struct SortPlan {
  bool ok = false;         // false: H1 < log2(sets) — a level-1 bin would straddle two scalar vectors; the caller refuses the MSM
  int H1 = 0, LB = 0;      // bits of a bucket id that pick the level-1 bin / the key inside it (H1 + LB = kbits)
  uint32_t nbins1 = 0;     // level-1 bins of all scalar vectors
  uint32_t nbins_set = 0;  // level-1 bins of one scalar vector (what the level-1 kernels see)
  uint32_t tile = 0;       // scalars per workgroup of the level-1 passes, a multiple of 256
  uint32_t nblocks = 0;    // tiles per scalar vector (<= 1536)
  size_t hist_n = 0;       // (bin, tile) counts + the total (== number of non-zero digits)
  uint32_t staged_sub = 0; // != 0: the staged level-1 scatter, in sub-rounds of this many scalars
  size_t staged_lds = 0;   // its dynamic LDS bytes
  size_t bin_lds = 0;      // dynamic LDS bytes of sort_bin_kernel
};

// n scalars per vector, W windows, `sets` scalar vectors (a power of two), kbits bits per bucket id.  forced_h1 > 0: the level-1
// bits asked for (ZKP_SORT_H1).  staged_enabled: ZKP_SORT_STAGED.
inline SortPlan sort_plan(size_t n, int W, int sets, int kbits, int forced_h1, bool staged_enabled) {
  SortPlan p;
  int lgs = 0;
  while ((1 << lgs) < sets) lgs++;
  const size_t E = n * (size_t)W * (size_t)sets;
  // level-1 bins: enough of them that a bin (E / bins entries on average) fits the level-2 kernel's LDS stage
  int H1 = 10;
  while (H1 < SORT_H1_MAX && (E >> H1) > SORT_BIN_TARGET) H1++;
  if (forced_h1 > 0) H1 = forced_h1 < SORT_H1_MAX ? forced_h1 : SORT_H1_MAX;
  if (H1 > kbits) H1 = kbits;
  if (kbits - H1 > SORT_L_MAX) H1 = kbits - SORT_L_MAX;
  p.ok = H1 >= lgs;
  if (!p.ok) return p;
  p.H1 = H1;
  p.LB = kbits - H1;
  p.nbins1 = 1u << H1;
  p.nbins_set = p.nbins1 >> lgs;
  // tiles: 2048 scalars, more for large MSMs so that the (bin x tile) count matrix stays small
  p.tile = SORT_SCALARS;
  while ((n + p.tile - 1) / p.tile > 1536) p.tile += 256;
  p.nblocks = (uint32_t)((n + p.tile - 1) / p.tile);
  p.hist_n = (size_t)p.nbins1 * p.nblocks + 1;
  // staged level-1 scatter: sub-rounds of `staged_sub` scalars whose entries fit the LDS stage; not for > 2048 level-1 bins (the
  // two counter arrays would leave one workgroup per CU) or very narrow windows
  if (staged_enabled && p.nbins_set <= 2048 && (size_t)256 * W * 8 <= SORT_STAGE_BYTES) {
    p.staged_sub = (uint32_t)(SORT_STAGE_BYTES / ((size_t)W * 8)) / 256 * 256;
    if (p.staged_sub > p.tile) p.staged_sub = p.tile;
    p.staged_lds = ((size_t)p.nbins_set + ((p.nbins_set + 3) & ~3u)) * 4 + (size_t)p.staged_sub * W * 8;
  }
  p.bin_lds = ((size_t)4 << p.LB) + 4 * (size_t)SORT_BIN_STAGE;
  return p;
}

// The task schedule of nb buckets and E entries, at most `cap` entries per task, in ONE buffer of 32-bit words.  A bucket of len
// entries becomes ceil(len / cap) tasks, so nb + E / cap + 1 bounds their number.
struct SchedLayout {
  uint32_t max_tasks = 0;
  size_t words = 0;                        // to allocate
  // word offsets
  size_t tcount = 0, toff = 0;             // nb + 1 words each (toff[nb] = number of tasks)
  size_t task_start = 0, task_len = 0, task_dst = 0, long_list = 0;   // max_tasks words each
  size_t tmeta = 0;                        // TM_WORDS words
  size_t desc_bytes = 0;                   // BYTE offset of the max_tasks 16-byte task descriptors, 16-byte aligned when the buffer is
};
inline SchedLayout sched_layout(uint32_t nb, size_t E, uint32_t cap) {
  SchedLayout s;
  s.max_tasks = nb + (uint32_t)(E / cap) + 1;
  s.words = (size_t)2 * (nb + 2) + (size_t)8 * s.max_tasks + TM_WORDS + 8;
  s.tcount = 0;
  s.toff = (size_t)nb + 2;
  s.task_start = s.toff + ((size_t)nb + 2);
  s.task_len = s.task_start + s.max_tasks;
  s.task_dst = s.task_len + s.max_tasks;
  s.long_list = s.task_dst + s.max_tasks;
  s.tmeta = s.long_list + s.max_tasks;
  s.desc_bytes = ((s.tmeta + TM_WORDS) * 4 + 15) & ~(size_t)15;
  return s;
}

}  // namespace zkp
