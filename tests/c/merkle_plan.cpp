// Prints the launch plan of fr_hash.hpp for every n of [argv[1], argv[2]]: one line "n tail_nodes lo:hi:tail ..." per n.
// tests/test_merkle_plan.py checks the lines.  Host only: the header names no HIP type.
#include <cstdio>
#include <cstdlib>

#include "fr_hash.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const uint64_t first = strtoull(argv[1], nullptr, 10), last = strtoull(argv[2], nullptr, 10);
  for (uint64_t n = first; n <= last; n++) {
    printf("%llu %u", (unsigned long long)n, zkp::HASH_TAIL_NODES);
    for (const zkp::MerkleLaunch& l : zkp::merkle_plan(n))
      printf(" %llu:%llu:%d", (unsigned long long)l.lo, (unsigned long long)l.hi, l.tail ? 1 : 0);
    printf("\n");
  }
  return 0;
}
