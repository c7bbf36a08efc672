// CPU print-out of the MSM sort and schedule geometry (ckb_zkp_amd/csrc/msm_sort_plan.hpp): includes that header and nothing else of
// the library.  argv: n W sets kbits forced_h1 staged(0|1) cap.  Prints one line of name=value pairs: the SortPlan ("ok=0" alone when
// the shape is refused), then the SchedLayout of nb = 2^kbits buckets and E = n * W * sets entries.
#include <cstdio>
#include <cstdlib>

#include "msm_sort_plan.hpp"

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  const size_t n = (size_t)strtoull(argv[1], nullptr, 10);
  const int W = atoi(argv[2]), sets = atoi(argv[3]), kbits = atoi(argv[4]), forced_h1 = atoi(argv[5]);
  const bool staged = atoi(argv[6]) != 0;
  const uint32_t cap = (uint32_t)strtoul(argv[7], nullptr, 10);
  const zkp::SortPlan p = zkp::sort_plan(n, W, sets, kbits, forced_h1, staged);
  if (!p.ok) return printf("ok=0\n"), 0;
  printf("ok=1 H1=%d LB=%d nbins1=%u nbins_set=%u tile=%u nblocks=%u hist_n=%zu staged_sub=%u staged_lds=%zu bin_lds=%zu", p.H1, p.LB,
         p.nbins1, p.nbins_set, p.tile, p.nblocks, p.hist_n, p.staged_sub, p.staged_lds, p.bin_lds);
  const zkp::SchedLayout s = zkp::sched_layout(1u << kbits, n * (size_t)W * (size_t)sets, cap);
  printf(" max_tasks=%u words=%zu tcount=%zu toff=%zu task_start=%zu task_len=%zu task_dst=%zu long_list=%zu tmeta=%zu desc_bytes=%zu\n",
         s.max_tasks, s.words, s.tcount, s.toff, s.task_start, s.task_len, s.task_dst, s.long_list, s.tmeta, s.desc_bytes);
  return 0;
}
