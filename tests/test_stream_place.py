"""CPU: the order in which a lane creates its streams (ckb_zkp_amd/csrc/stream_place.hpp, used by zkp_ctx_create_ex).

tests/c/stream_place.cpp includes that header and nothing else of the library and prints stream_role_at for every queue count,
lane and slot.  The queue of a stream is its cumulative creation index (lane * 4 + slot) mod the queue count: ROCm hands hardware
queues out round-robin in stream-creation order.

What must hold with 1, 2 or 4 queues (the counts that divide the four roles), for every lane count 1..8:
  * main of lane l + 1 shares a queue with ws1 of lane l;
  * the stream that follows main of lane l on its queue is ws3 of lane l + 1.  With four queues that is literally the next stream
    created on that queue.  With one or two queues a queue holds several streams of the SAME lane, so the next stream created on
    main's queue is usually one of lane l itself and no creation order can change that; there the check is on the stream one whole
    lane (four creations) later, which shares main's queue at every queue count dividing four;
  * consecutive lanes' mains are on different queues (not at one queue, where everything shares the only queue).
With every other queue count the order is the identity: the placement measured at 8, 16 and 32 queues stays.
(ROCm 7.2.0 was seen to cycle through its four queues downwards, 4, 3, 2, 1, from a process's fifth stream on, the first four having
opened them upwards — profiles/stream_placement_trace.txt.  Every property above compares streams whose creation indices are congruent
modulo the queue count, so it holds for a cycle in either direction; "index mod queues" is the model, not the queue's name.)

ZKP_C_DRIVER_FLAGS="-fsanitize=address,undefined" builds the program sanitized, as for tests/c/tune_table.cpp."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ckb_zkp_amd" / "csrc"
SRC = ROOT / "tests" / "c" / "stream_place.cpp"
OUT = ROOT / "tests" / "c" / "build" / "stream_place"

N_ROLES, MAX_QUEUES, MAX_LANES = 4, 32, 8
MAIN, WS1, WS3 = 0, 1, 3
ROTATED = (1, 2, 4)


@pytest.fixture(scope="module")
def role_at():
    """{(queues, lane, slot): role} as the header computes it"""
    OUT.parent.mkdir(exist_ok=True)
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{CSRC}", str(SRC), "-o", str(OUT)]
    r = subprocess.run(cmd + os.environ.get("ZKP_C_DRIVER_FLAGS", "").split(), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(OUT), str(N_ROLES), str(MAX_QUEUES), str(MAX_LANES)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
    table = {}
    for line in out.stdout.splitlines():
        q, lane, slot, role = map(int, line.split())
        table[q, lane, slot] = role
    assert len(table) == (MAX_QUEUES + 1) * MAX_LANES * N_ROLES
    return table


def placement(role_at, queues, lanes):
    """[(queue, lane, role)] in creation order, and {(lane, role): position in that list}"""
    order = []
    for lane in range(lanes):
        for slot in range(N_ROLES):
            order.append(((lane * N_ROLES + slot) % queues, lane, role_at[queues, lane, slot]))
    return order, {(lane, role): i for i, (_, lane, role) in enumerate(order)}


@pytest.mark.parametrize("queues", range(1, MAX_QUEUES + 1))
def test_every_lane_creates_each_role_once(role_at, queues):
    for lane in range(MAX_LANES):
        assert sorted(role_at[queues, lane, slot] for slot in range(N_ROLES)) == list(range(N_ROLES)), lane


@pytest.mark.parametrize("queues", ROTATED)
@pytest.mark.parametrize("lanes", range(1, MAX_LANES + 1))
def test_roles_rotate_over_the_queues_when_the_queue_count_divides_the_roles(role_at, queues, lanes):
    order, pos = placement(role_at, queues, lanes)
    queue_of = {(lane, role): q for q, lane, role in order}
    for lane in range(lanes):
        assert role_at[queues, lane, (lane + MAIN) % N_ROLES] == MAIN                 # (slot - lane) mod 4, not (slot + lane) mod 4
    for lane in range(lanes - 1):
        assert queue_of[lane + 1, MAIN] == queue_of[lane, WS1], lane
        q = queue_of[lane, MAIN]
        later = [(l, r) for i, (qq, l, r) in enumerate(order) if qq == q and i > pos[lane, MAIN]]
        if queues == N_ROLES:
            assert later[0] == (lane + 1, WS3), lane                                  # the very next stream of that queue
        one_lane_on = order[pos[lane, MAIN] + N_ROLES]
        assert one_lane_on == (q, lane + 1, WS3) and (lane + 1, WS3) in later, lane
        if queues > 1:
            assert queue_of[lane + 1, MAIN] != q, lane


@pytest.mark.parametrize("queues", [q for q in range(0, MAX_QUEUES + 1) if q not in ROTATED])
def test_every_other_queue_count_keeps_the_lane_major_order(role_at, queues):
    for lane in range(MAX_LANES):
        for slot in range(N_ROLES):
            assert role_at[queues, lane, slot] == slot, (lane, slot)


def test_the_context_creates_its_streams_in_that_order():
    """capi.hip asks the header for every stream it creates, reads the queue count once through env_num with 4 as the value of an unset
    variable, and nothing in the library writes the process environment."""
    capi = (CSRC / "capi.hip").read_text()
    assert '#include "stream_place.hpp"' in capi
    assert len(re.findall(r'env_num\("GPU_MAX_HW_QUEUES", 4\)', capi)) == 1
    assert "stream_role_at(" in capi
    header = (CSRC / "stream_place.hpp").read_text()
    assert "#include" not in header                                                   # nothing of HIP, nothing at all
    for p in sorted(CSRC.iterdir()):
        if p.suffix in (".hip", ".hpp", ".cpp", ".inc"):
            assert not re.search(r"\b(setenv|putenv|unsetenv)\s*\(", p.read_text()), p.name
