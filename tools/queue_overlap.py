#!/usr/bin/env python3
"""Where the streams of the pipelined Groth16 batch sit on the hardware queues, and whether consecutive proofs overlap: read from a
rocprofv3 kernel-trace database of `bench.py --gpus 1 --steps K --warmup W`.

    rocprofv3 --kernel-trace -d DIR -o t -- python bench.py --gpus 1 --steps 24 --warmup 8
    python tools/queue_overlap.py DIR/.../t_results.db [--steps 24] [--lanes 8] [--group 1] [--label before]

Proofs are delimited by the launches of assemble_g1_part2_kernel: one per proof, the last kernel on the proof's main stream.  The
streams that launch prover kernels are grouped four by four in the order of their ids (a lane's four streams are created
together); a proof is everything its lane's streams start after the lane's previous part 2 and up to its own.  The timed batch is
the last K proofs; the steady-state window leaves out its first and last `lanes` proofs (pipeline fill and drain).
With fused proof groups (groth16.hip ZKP_PROOF_FUSE) one part 2 launch closes --group proofs: the units between two launches are
groups, K / group of them are timed, `lanes` groups are left out at either end, and the per-proof figures divide by the group size.

Prints, for that window: per hardware-queue id the stream ids seen on it in order of first use (and which lane / role each is),
the union coverage of the accumulate_kernel intervals, the largest number of kernels in flight, and for every pair of consecutive
proofs whether a kernel of proof k + 1 started before the last final_kernel / assemble_g1_part2_kernel of proof k ended.  The input
copies that open a proof (witness, r, s) are counted apart: they wait for nothing and run when the host enqueues them, several
proofs ahead, wherever their stream sits."""
import argparse
import re
import sqlite3
from collections import defaultdict

ROLES = ("main", "ws1", "ws2", "ws3")


def load(path):
    db = sqlite3.connect(path)
    cur = db.cursor()
    syms = {r[0]: re.sub(r"\(.*", "", r[1]) for r in cur.execute("select id, kernel_name from rocpd_info_kernel_symbol")}
    rows = cur.execute("select kernel_id, start, end, queue_id, stream_id from rocpd_kernel_dispatch order by start").fetchall()
    return [(syms.get(k, str(k)), s, e, q, st) for k, s, e, q, st in rows]


def short(name):
    for m in re.finditer(r"\d+", name):                       # mangled: <length><identifier>
        ident = name[m.end():m.end() + int(m.group())]
        if ident.endswith("_kernel"):
            return ident
    m = re.search(r"([A-Za-z_][A-Za-z_0-9]*_kernel)", name)
    return m.group(1) if m else name[:32]


def role_of(names):
    """which of a lane's four streams launched these kernels (groth16.hip: ws1: A -> L | ws2: B2 | ws3: B1, then part 1 | main: witness map -> H, part 2)"""
    if any("assemble_g1_part2_kernel" in n for n in names):
        return "main"
    if any("assemble_g1_part1_kernel" in n for n in names):
        return "ws3"
    if any("assemble_g2" in n or ("accumulate_kernel" in n and ("Fp2" in n or "c02" in n or "c12" in n)) for n in names):
        return "ws2"
    return "ws1"


def union(intervals, a, b):
    """(time covered by at least one interval, largest number of intervals open at once) inside [a, b]"""
    ev = sorted([(max(s, a), 1) for s, e in intervals if e > a and s < b] + [(min(e, b), -1) for s, e in intervals if e > a and s < b])
    busy, depth, peak, last = 0, 0, 0, a
    for t, d in ev:
        if depth > 0:
            busy += t - last
        depth += d
        peak = max(peak, depth)
        last = t
    return busy, peak


def analyse(rows, steps, lanes, label, group=1):
    out = []
    part2 = [r for r in rows if "assemble_g1_part2_kernel" in r[0]]
    proofs_timed = steps
    steps = steps // group                                   # units (groups of `group` proofs) from here on
    if len(part2) < steps:
        raise SystemExit(f"{len(part2)} assemble_g1_part2_kernel launches in the trace, fewer than --steps {proofs_timed} / --group {group}")
    t_first = part2[-steps][1]
    # the streams of the prover: whatever launched an accumulate or either half of the assembly during the timed batch
    prover = sorted({st for n, s, e, q, st in rows if s >= t_first - 5e7 and
                     ("accumulate_kernel" in n or "assemble_g1_part" in n)})
    if len(prover) < 4:
        raise SystemExit(f"the trace names {len(prover)} stream id(s) for the prover's kernels: kernels cannot be attributed to proofs")
    lane_of = {st: i // 4 for i, st in enumerate(prover)}
    n_lanes = (len(prover) + 3) // 4
    by_stream = defaultdict(list)
    for r in rows:
        if r[4] in lane_of:
            by_stream[r[4]].append(r)
    # proofs: per lane, cut at the end of every part 2 on one of the lane's streams
    proofs = []                                              # (part2 end, lane, [rows])
    for lane in range(n_lanes):
        mine = sorted((r for st in prover if lane_of[st] == lane for r in by_stream[st]), key=lambda r: r[1])
        cur = []
        for r in mine:
            cur.append(r)
            if "assemble_g1_part2_kernel" in r[0]:
                proofs.append((r[2], lane, cur))
                cur = []
    proofs.sort(key=lambda p: p[0])
    timed = proofs[-steps:]
    skip = lanes if steps - 2 * lanes >= 4 else 0
    steady = timed[skip:len(timed) - skip] if skip else timed
    a = timed[skip - 1][0] if skip else min(r[1] for r in steady[0][2])      # from the end of the proof before the first one
    b = steady[-1][0]
    sel = [r for r in rows if r[2] > a and r[1] < b]
    wall = b - a
    out.append(f"## {label}")
    unit = "proofs" if group == 1 else f"groups of {group} proofs"
    n_proofs = len(steady) * group
    out.append(f"timed batch: the last {steps} of {len(part2)} {unit} in the trace; steady-state window: {unit} {skip + 1}..{len(timed) - skip} "
               f"of the batch, {wall / 1e6:.2f} ms, {n_proofs} proofs = {wall / 1e6 / n_proofs:.3f} ms per proof under the tracer")
    launches = sum(1 for r in sel if r[4] in lane_of and "copyBuffer" not in r[0])
    out.append(f"kernel launches on the prover's streams in the window (copies left out): {launches} = {launches / n_proofs:.1f} per proof")
    out.append(f"prover streams: {len(prover)} in {n_lanes} lanes (ids {prover[0]}..{prover[-1]})" if prover else "no prover streams")

    # --- placement
    out.append("hardware queue id: stream ids in order of first use in the window (lane:role)")
    names_of = defaultdict(set)
    for n, s, e, q, st in sel:
        names_of[st].add(n)
    queues = defaultdict(list)
    for n, s, e, q, st in sel:
        if st not in queues[q]:
            queues[q].append(st)
    role = {st: role_of(names_of[st]) for st in prover if st in names_of}
    mains = {}
    for q in sorted(queues):
        txt = " ".join(f"{st}({lane_of[st]}:{role[st]})" if st in lane_of else f"{st}(-)" for st in queues[q])
        roles_here = sorted({role[st] for st in queues[q] if st in role}, key=ROLES.index)
        out.append(f"  queue {q}: {txt}   roles: {','.join(roles_here) if roles_here else '-'}")
        for st in queues[q]:
            if role.get(st) == "main":
                mains[lane_of[st]] = q
    multi = sorted(st for st in lane_of if sum(st in v for v in queues.values()) > 1)
    if multi:
        out.append(f"  streams seen on more than one queue: {multi}")
    diff = sum(1 for l in range(n_lanes) if l in mains and (l + 1) % n_lanes in mains and mains[l] != mains[(l + 1) % n_lanes])
    out.append(f"  main streams of consecutive lanes on different queue ids: {diff} of {n_lanes} pairs "
               f"(main stream's queue per lane: {[mains.get(l) for l in range(n_lanes)]})")

    # --- coverage
    acc_busy, acc_peak = union([(s, e) for n, s, e, q, st in sel if "accumulate_kernel" in n], a, b)
    any_busy, any_peak = union([(s, e) for n, s, e, q, st in sel], a, b)
    out.append(f"accumulate_kernel union coverage: {acc_busy / wall:.3f} of the window (at most {acc_peak} at once)")
    out.append(f"any kernel: union coverage {any_busy / wall:.3f}; largest number of kernels in flight: {any_peak}")

    # --- do consecutive proofs overlap?  (the three input copies of a proof need nothing that precedes them and carry no barrier bit:
    # they run when the host enqueues them, several proofs ahead, under every placement, and are counted apart)
    def is_copy(r):
        return "copyBuffer" in r[0]

    out.append("consecutive proofs (k, k+1): lead = end of proof k's last final_kernel / part 2 minus start of the first kernel of proof k+1 "
               "that is not an input copy")
    n_over, n_acc, leads, early_counts = 0, 0, [], []
    for (e0, l0, r0), (e1, l1, r1) in zip(steady, steady[1:]):
        last_end = max(r[2] for r in r0 if "final_kernel" in r[0] or "assemble_g1_part2_kernel" in r[0])
        work = [r for r in r1 if not is_copy(r)]
        early = [r for r in work if r[1] < last_end]
        copies = sum(1 for r in r1 if is_copy(r) and r[1] < last_end)
        lead = (last_end - min(r[1] for r in work)) / 1e6
        leads.append(lead)
        early_counts.append(len(early))
        n_over += bool(early)
        n_acc += any("accumulate_kernel" in r[0] for r in early)
        what = ", ".join(sorted({short(r[0]) for r in early})[:8])
        out.append(f"  lanes {l0}->{l1} (main on queues {mains.get(l0)}->{mains.get(l1)}): lead {lead:7.3f} ms, {len(early):4d} of {len(work):4d} kernels of k+1 "
                   f"start before k's last kernel ends, + {copies} input copies" + (f" ({what})" if early else ""))
    if leads:
        out.append(f"pairs in which a kernel of proof k+1 starts before proof k's last kernel ends: {n_over} of {len(leads)}; "
                   f"an accumulate_kernel of k+1 among them: {n_acc}; mean lead {sum(leads) / len(leads):.3f} ms, "
                   f"mean kernels of k+1 started early {sum(early_counts) / len(early_counts):.1f}")
    return "\n".join(out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("db")
    ap.add_argument("--steps", type=int, default=24, help="timed proofs of the traced bench run")
    ap.add_argument("--lanes", type=int, default=8, help="proofs left out at either end of the timed batch")
    ap.add_argument("--group", type=int, default=1, help="proofs closed by one assemble_g1_part2_kernel launch (fused groups)")
    ap.add_argument("--label", default="trace")
    a = ap.parse_args()
    print(analyse(load(a.db), a.steps, a.lanes, a.label, a.group))
