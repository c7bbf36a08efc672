// Prints the plan of pedersen.hpp for one (curve, cols): tests/test_pedersen_plan.py compares it with a Python restatement.
// Host only: the header names no HIP type.
#include <cstdio>
#include <cstdlib>

#include "pedersen.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const int curve = atoi(argv[1]);
  const uint32_t cols = (uint32_t)strtoul(argv[2], nullptr, 10);
  const zkp::PedersenPlan p = zkp::pedersen_plan(curve, cols);
  printf("c=%u W=%u nb=%u G=%u S=%u g=%u lds_bytes=%u bk_bytes=%u lanes=%d slots=%d max_entries=%u max_gens=%u lds_max=%u launches=%d "
         "row_chunk=%u vecmat_threads=%u\n",
         p.c, p.W, p.nb, p.G, p.S, p.g, p.lds_bytes, zkp::pedersen_bk_bytes(curve), zkp::PED_LANES, zkp::PED_SLOTS, zkp::PED_MAX_ENTRIES,
         zkp::PED_MAX_GENS, zkp::PED_LDS_MAX, zkp::PED_LAUNCHES, zkp::VECMAT_ROW_CHUNK, zkp::VECMAT_THREADS);
  return 0;
}
