#!/usr/bin/env python3
"""The SHA-256 entries on one MI355X.  HIP events around each alternative (zkp_timer_*), every window ends in a synchronise; after
one warm-up the alternatives take turns inside one loop of one process, medians of --reps.  One JSON line per row;
`python tools/sha256_bench.py > profiles/sha256_bench.txt`.

  * digests: zkp_sha256_dev over n = 2^10 .. 2^20 messages of 64 bytes (two compressions each): time and digests per second.
  * tree: zkp_sha256_merkle_tree_dev at 2^12, 2^16, 2^20 leaves with its launch count (one per depth of inner nodes).
  * witness: sha256.witness_dev for circuits.Sha256Merkle at --depth (20), as trace and expand separately, against the upload of
    the finished z alone and the host synthesis (with the Montgomery encoding) that precedes that upload.  The expand's written
    bytes per second stand against zkp_bench_hbm_copy, the copy floor the other benches use.

    python tools/sha256_bench.py [--reps 5] [--logs 10 12 14 16 18 20] [--tree-logs 12 16 20] [--depth 20] [--curve bn254]
Runs on the GPU only: creating the context fails without one."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import circuits, codec, merkle  # noqa: E402
from ckb_zkp_amd import sha256 as S  # noqa: E402
from ckb_zkp_amd.api import Context  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402


def timed(ctx, fns, reps):
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ctx.timer_start()
            fn()
            ts[name].append(ctx.timer_stop_ms())
    return {name: float(np.median(v)) for name, v in ts.items()}


def digests_case(ctx, log, reps, d_msgs, d_out, host_msgs):
    n = 1 << log

    def run():
        ctx.sha256_dev(d_msgs, n, 64, d_out)
        ctx.sync()
    run()
    got = np.zeros(32, dtype=np.uint8)
    ctx.d2h(got, d_out + 32 * (n - 1))
    same = got.tobytes() == hashlib.sha256(host_msgs[64 * (n - 1):64 * n].tobytes()).digest()
    ms = timed(ctx, {"digests": run}, reps)["digests"]
    return dict(case="digests", n=n, message_bytes=64, reps=reps, last_digest_matches_hashlib=bool(same), ms=round(ms, 4),
                mdigests_per_s=round(n / (ms * 1e-3) / 1e6, 2), gcompressions_per_s=round(2 * n / (ms * 1e-3) / 1e9, 3))


def tree_case(ctx, log, reps, d_nodes):
    n = 1 << log

    def run():
        ctx.sha256_merkle_tree_dev(d_nodes, n)
        ctx.sync()
    run()
    ms = timed(ctx, {"tree": run}, reps)["tree"]
    return dict(case="tree", n=n, reps=reps, launches=merkle.depth(n - 2) + 1, ms=round(ms, 4),
                mmerges_per_s=round((n - 1) / (ms * 1e-3) / 1e6, 2))


def witness_case(ctx, c, depth, reps):
    rng = np.random.default_rng(20)
    index = (1 << depth) - 1 + int(rng.integers(0, 1 << depth))
    leaf = rng.bytes(32)
    lemmas = [rng.bytes(32) for _ in range(depth)]
    msgs = merkle.membership_messages(index, leaf, lemmas)
    root = hashlib.sha256(msgs[-1]).digest()
    t0 = time.perf_counter()
    cs, plan = S.synthesize(circuits.Sha256Merkle(index, leaf, lemmas, root), c, True)
    synth_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    z = codec.fr_to_mont(cs.full_assignment(), c)
    encode_s = time.perf_counter() - t0
    m, W = len(plan.codes), plan.words_per_msg
    d_m, pd = ctx.to_device(np.frombuffer(b"".join(msgs), dtype=np.uint8)), S.upload_plan(ctx, plan)
    d_t, d_z = ctx.dev_alloc(4 * W * depth), ctx.dev_alloc(z.nbytes)
    try:
        def upload():
            ctx.h2d(d_z, z)
            ctx.sync()

        def trace():
            ctx.sha256_trace_dev(d_m, depth, 64, d_t)
            ctx.sync()

        def expand():
            ctx.fr_bits_expand_dev(c, d_t, W, depth, 1, pd.codes_dev, m, pd.max_v, d_z, m)
            ctx.sync()

        def whole():
            ctx.dev_free(S.witness_dev(ctx, c, pd, d_m, 1))
        upload()
        trace()
        expand()
        whole()
        got = np.zeros_like(z)
        ctx.d2h(got, d_z)
        med = timed(ctx, {"upload": upload, "trace": trace, "expand": expand, "witness_dev": whole}, reps)
        copy_gbs = ctx.bench_hbm_copy()
    finally:
        for p in (d_m, d_t, d_z):
            ctx.dev_free(p)
        pd.free()
    return dict(case="witness", curve=c.name, depth=depth, constraints=cs.num_constraints(), elements=m, z_bytes=int(z.nbytes), reps=reps,
                same_words=bool(np.array_equal(got, z)), host_synthesis_s=round(synth_s, 2), host_encode_s=round(encode_s, 2),
                upload_ms=round(med["upload"], 3), trace_ms=round(med["trace"], 3), expand_ms=round(med["expand"], 3),
                witness_dev_ms=round(med["witness_dev"], 3), expand_written_gb_per_s=round(z.nbytes / (med["expand"] * 1e-3) / 1e9, 1),
                hbm_copy_gb_per_s=round(copy_gbs, 1),
                note="trace: one lane per message, `depth` lanes in all; witness_dev: both launches, the two allocations and their release")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logs", type=int, nargs="*", default=[10, 12, 14, 16, 18, 20])
    ap.add_argument("--tree-logs", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--curve", default="bn254")
    args = ap.parse_args()
    ctx = Context(0)                                               # no GPU: this raises
    reps = max(args.reps, 3)
    n_max = 1 << max(args.logs + args.tree_logs + [10])
    rng = np.random.default_rng(7)
    host_msgs = np.frombuffer(rng.bytes(64 * n_max), dtype=np.uint8)
    d_msgs, d_out = ctx.to_device(host_msgs), ctx.dev_alloc(32 * n_max)
    try:
        for log in args.logs:
            print(json.dumps(digests_case(ctx, log, reps, d_msgs, d_out, host_msgs)), flush=True)
        for log in args.tree_logs:                                 # the message bytes as 2 n - 1 items: the last n are the leaves
            print(json.dumps(tree_case(ctx, log, reps, d_msgs)), flush=True)
    finally:
        ctx.sync()
        ctx.dev_free(d_msgs)
        ctx.dev_free(d_out)
    if args.depth:
        print(json.dumps(witness_case(ctx, get_curve(args.curve), args.depth, reps)), flush=True)


if __name__ == "__main__":
    main()
