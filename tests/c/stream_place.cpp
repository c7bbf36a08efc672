// The stream-creation order of ckb_zkp_amd/csrc/stream_place.hpp, stand-alone (host compiler, no GPU, nothing else of the library):
//     stream_place <n_roles> <max_queues> <max_lanes>
// prints one line "queues lane slot role" for every queue count 0..max_queues, lane and slot.  tests/test_stream_place.py holds the
// properties the table must have.
#include <cstdio>
#include <cstdlib>

#include "stream_place.hpp"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const int n_roles = atoi(argv[1]), max_queues = atoi(argv[2]), max_lanes = atoi(argv[3]);
  if (n_roles < 1 || max_queues < 1 || max_lanes < 1) return 2;
  for (int q = 0; q <= max_queues; q++)
    for (int lane = 0; lane < max_lanes; lane++)
      for (int slot = 0; slot < n_roles; slot++)
        printf("%d %d %d %d\n", q, lane, slot, zkp::stream_role_at(lane, slot, n_roles, q));
  return 0;
}
