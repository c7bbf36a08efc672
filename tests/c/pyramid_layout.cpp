// CPU check of the bucket-reduction pyramid layout (ckb_zkp_amd/csrc/msm_pyramid.hpp): includes that header and nothing else of the
// library.  argv: nb_set S top_max chunk fused(0|1).  Prints "ok l_top=<l> end=<elements>" or the first violated property.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "msm_pyramid.hpp"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const uint32_t nb_set = (uint32_t)strtoul(argv[1], nullptr, 10), S = (uint32_t)strtoul(argv[2], nullptr, 10);
  const uint32_t top_max = (uint32_t)strtoul(argv[3], nullptr, 10), chunk = (uint32_t)strtoul(argv[4], nullptr, 10);
  const bool fused = atoi(argv[5]) != 0;
  int L = 0;
  while ((1u << L) < nb_set) L++;
  const zkp::PyramidLevels p = zkp::pyramid_levels(nb_set, S, L, fused, top_max, chunk);
  const uint32_t cap = 2 * S * nb_set;                          // the bucket buffer holds 2 nb + 1 points
  if (p.end > cap) return printf("end %u beyond the buffer %u\n", p.end, cap), 1;
  std::vector<int> owner(cap, -1);                              // element -> set * 64 + level
  for (int l = 0; l <= L; l++) {
    if (p.cnt[l] != nb_set >> l) return printf("level %d holds %u entries per set\n", l, p.cnt[l]), 1;
    for (uint32_t g = 0; g < S; g++) {
      const uint64_t lo = (uint64_t)p.off[l] + (uint64_t)g * p.step[l];
      if (lo + p.cnt[l] > p.end) return printf("set %u level %d ends at %llu, beyond %u\n", g, l, (unsigned long long)(lo + p.cnt[l]), p.end), 1;
      for (uint32_t i = 0; i < p.cnt[l]; i++) {
        if (owner[lo + i] >= 0) return printf("set %u level %d overlaps set %d level %d at %llu\n", g, l, owner[lo + i] / 64, owner[lo + i] % 64, (unsigned long long)(lo + i)), 1;
        owner[lo + i] = (int)g * 64 + l;
      }
    }
  }
  if (S == 1)                                                   // the plain layout: every level directly behind the one before
    for (int l = 0; l < L; l++)
      if (p.off[l + 1] != p.off[l] + p.cnt[l]) return printf("S = 1: level %d not directly behind level %d\n", l + 1, l), 1;
  if (p.l_top >= 0) {
    // pair_top_body: set g reads its cnt entries at off[l_top] + g * cnt and writes level l_top + 1 at off[l_top] + (S + g) * cnt,
    // every further level directly behind its predecessor
    if (p.step[p.l_top] != p.top_cnt || p.cnt[p.l_top] != p.top_cnt) return printf("top input level is not side by side\n"), 1;
    for (uint32_t g = 0; g < S; g++) {
      uint64_t at = (uint64_t)p.off[p.l_top] + (uint64_t)(S + g) * p.top_cnt;
      for (int l = p.l_top + 1; l <= L; l++) {
        if ((uint64_t)p.off[l] + (uint64_t)g * p.step[l] != at) return printf("set %u level %d is not where pair_top writes it\n", g, l), 1;
        at += p.cnt[l];
      }
    }
  }
  printf("ok l_top=%d end=%u\n", p.l_top, p.end);
  return 0;
}
