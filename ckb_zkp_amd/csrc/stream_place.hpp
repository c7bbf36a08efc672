// In which order a lane creates its streams (zkp_ctx_create_ex).  Pure host arithmetic, nothing of HIP: tests/c/stream_place.cpp
// includes this header alone.
//
// ROCm hands hardware queues out round-robin in stream-creation order: streams whose creation numbers are congruent modulo
// hw_queues share a queue (ROCm 7.2.0 cycles downwards from the process's fifth stream on, after the first four have opened the
// queues upwards; only the congruence is relied on).  A lane has n_roles streams (role 0 = main, 1 .. n_roles - 1 = the MSM
// workspaces).  Created role by role in every lane, with hw_queues dividing n_roles, all main streams share ONE queue, and a queue
// starts a packet that carries the barrier bit only after everything submitted to it earlier: proof k + 1 opens with kernels on its
// main stream (scalar tail, fork event, witness map), which then sit behind the join, assembly and read-back that close proof k on
// the same queue, and consecutive proofs do not overlap (profiles/stream_placement_trace.txt).
#pragma once

namespace zkp {

// The role lane `lane` creates as its `slot`-th stream.
//   hw_queues divides n_roles (1, 2, 4 queues for 4 roles): the roles are rotated by the lane index, so that role r of lane l is
//     stream number l * n_roles + (r + l) mod n_roles and shares a queue with every stream of slot (r + l) mod hw_queues.  Main of lane
//     l + 1 then follows ws1 of lane l (A and L's accumulate: done early in a proof), and what follows main of lane l is ws3 of lane
//     l + 1 (s*g_a + r*g1_b: what a proof needs last).  Rotating the other way puts A of proof k + 1 behind the join of proof k.
//   otherwise (8, 16, 32 queues; anything else): role = slot in every lane, the order those counts were measured with.
inline int stream_role_at(int lane, int slot, int n_roles, int hw_queues) {
  if (hw_queues <= 0 || n_roles <= 0 || n_roles % hw_queues != 0) return slot;
  return ((slot - lane) % n_roles + n_roles) % n_roles;
}

}  // namespace zkp
