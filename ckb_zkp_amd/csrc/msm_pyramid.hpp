// Where the levels of the bucket-reduction pyramid live (msm.hip K8).  Pure host code without HIP: tests/c/pyramid_layout.cpp checks
// on the CPU that no two (set, level) regions overlap and that everything stays inside the bucket buffer.
//
// Level 0 = the buckets, level l + 1 = pairwise sums of level l, level L = the root.  With S bucket sets of a fused MSM (msm.hip
// `sets`) a level holds the S sets side by side — up to and including the level the one-workgroup top (pair_top) starts from.
// pair_top stores each level directly behind its predecessor, so the top of set g writes its levels into a region of its own,
// top_cnt entries long, behind the S sets of its input level.  S == 1 gives the plain layout: every level behind the one before.
#pragma once
#include <stdint.h>

namespace zkp {

struct PyramidLevels {
  int L = 0;               // levels 0 .. L (L = the root, one entry per set)
  int l_top = -1;          // level the fused top starts from (it produces levels l_top + 1 .. L); -1: no fused top
  uint32_t top_cnt = 0;    // entries per set at level l_top
  uint32_t off[27] = {};   // element offset of set 0's level l
  uint32_t cnt[27] = {};   // entries per set at level l
  uint32_t step[27] = {};  // set g's level l starts g * step[l] elements behind set 0's
  uint32_t end = 0;        // elements used in all
};

// nb_set: buckets per set (a power of two), L = log2(nb_set).  fused_top: the top may be fused with the segmented sums (pair_top and
// pair_top_fuse_seg on); it starts at the level with top_max entries per set, or at level 0 when there are fewer, provided its
// odd entries fit one segmented-sum block (cnt / 2 <= chunk).
inline PyramidLevels pyramid_levels(uint32_t nb_set, uint32_t S, int L, bool fused_top, uint32_t top_max, uint32_t chunk) {
  PyramidLevels p;
  p.L = L;
  uint32_t off = 0, cnt = nb_set;
  for (int l = 0; l <= L; l++) {
    const bool in_top = p.l_top >= 0 && l > p.l_top;     // inside the per-set regions
    p.off[l] = off;
    p.cnt[l] = cnt;
    p.step[l] = in_top ? p.top_cnt : cnt;
    if (l < L && fused_top && p.l_top < 0 && cnt <= top_max && (cnt == top_max || l == 0) && cnt / 2 <= chunk) {
      p.l_top = l;
      p.top_cnt = cnt;
    }
    off += in_top ? cnt : S * cnt;
    cnt /= 2;
  }
  // the last region of the top is top_cnt entries long although its levels fill top_cnt - 1 of them
  p.end = p.l_top >= 0 ? p.off[p.l_top] + 2 * S * p.top_cnt : off;
  return p;
}

}  // namespace zkp
