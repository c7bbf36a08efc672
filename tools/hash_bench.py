#!/usr/bin/env python3
"""The hash and Merkle entries on one MI355X.  HIP events around each alternative (zkp_timer_*), every window ends in a
synchronise; after a warm-up the alternatives take turns inside one loop of one process, medians of --reps.  One JSON line per
row; `python tools/hash_bench.py > profiles/hash_bench.txt`.

  * blocks: zkp_fr_hash_blocks_dev per kind and curve at n = 2^10, 2^14, 2^18, 2^20: time, Fr products per second by the exact
    product count of the schedule (zkp_hash_params_info), and that rate over zkp_bench_mulmod's Fr rate of the same run.
    Schedules: MiMC-5, MiMC-322, Poseidon 91 rounds with one partial round, Rescue R = 22; constants from the PRF of circuits.py.
  * mimc_vs_composition: MiMC-5 and MiMC-322 against the composition the exports offered before (per round VEC_ADDC, VEC_MUL,
    VEC_MUL, VEC_ADD of zkp_fr_vec_op_dev), the composition twice per turn (its own spread); both give the same words.
  * tree: zkp_fr_merkle_tree_dev with Poseidon and ZKP_MERGE_BLOCK at n = 2^12, 2^16, 2^20: the total and the tail launch alone
    (a tree of 512 leaves is exactly the tail: nine depths in one workgroup).  --only-tree LOG builds that one tree a few times and
    nothing else, for a kernel trace in a run of its own.
  * witness: hashes.mimc_chain_witness_dev at S = samples_for_domain(20) against the host loop of circuits.mimc_chain_instance
    and the upload of z that it replaces.

    python tools/hash_bench.py [--reps 5] [--logs 10 14 18 20] [--tree-logs 12 16 20] [--curves bn254 bls12_381] [--witness-curves bn254]
                                 [--only-tree LOG]
Runs on the GPU only: creating the context fails without one."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ckb_zkp_amd import codec, hashes, merkle  # noqa: E402
from ckb_zkp_amd.api import VEC_ADD, VEC_ADDC, VEC_MUL, Context  # noqa: E402
from ckb_zkp_amd.circuits import MIMC_ROUNDS, mimc_chain_instance, prf_field_elements, samples_for_domain  # noqa: E402
from ckb_zkp_amd.params import get_curve  # noqa: E402


def rand_fr(rng, c, n):
    """n reduced values as Montgomery words (any words below r are a valid vector)"""
    k = np.frombuffer(rng.bytes(32 * n), dtype=np.uint64).reshape(-1, 4).copy()
    k[:, 3] &= np.uint64((1 << (c.r.bit_length() - 193)) - 1)
    return k


def timed(ctx, fns, reps):
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ctx.timer_start()
            fn()
            ts[name].append(ctx.timer_stop_ms())
    return {name: float(np.median(v)) for name, v in ts.items()}


def rows3(vals, n):
    return [vals[3 * i:3 * i + 3] for i in range(n)]


def make_params(ctx, c):
    r = c.r
    v = prf_field_elements(0x4A54, 4096, r)
    return {
        "mimc5": hashes.HashParams.mimc(ctx, c, v[:5]),
        "mimc322": hashes.HashParams.mimc(ctx, c, v[:322]),
        "poseidon91": hashes.HashParams.poseidon(ctx, c, rows3(v, 91), rows3(v[300:], 3), hashes.poseidon_reference_schedule(91, 8)),
        "rescue22": hashes.HashParams.rescue(ctx, c, rows3(v, 45), rows3(v[300:], 3)),
    }, v


def blocks_case(ctx, c, name, hp, log, reps, fr_rate, d_l, d_r, d_o):
    n = 1 << log

    def run():
        ctx.fr_hash_blocks_dev(hp.handle, d_l, d_r, n, d_o)
        ctx.sync()
    run()
    ms = timed(ctx, {"blocks": run}, reps)["blocks"]
    products = hp.info()["products"]
    rate = n * products / (ms * 1e-3) / 1e9
    return dict(case="blocks", curve=c.name, hash=name, n=n, reps=reps, ms=round(ms, 4), products_per_block=int(products),
                gproducts_per_s=round(rate, 2), mulmod_gproducts_per_s=round(fr_rate, 1), of_mulmod=round(rate / fr_rate, 3))


def composition_case(ctx, c, name, hp, consts, log, reps, d_l, d_r, d_o, d_t, d_u):
    """the composition: per round t = xl + c (ADDC), u = t t (MUL), u = u t (MUL), u = u + xr (ADD), then (xl, xr) <- (u, xl) by
    rotating three buffers; 4 launches a round"""
    n = 1 << log
    cw = codec.fr_to_mont(consts, c)
    d_a, d_b = ctx.dev_alloc(32 * n), ctx.dev_alloc(32 * n)
    try:
        def fused():
            ctx.fr_hash_blocks_dev(hp.handle, d_l, d_r, n, d_o)
            ctx.sync()

        def composed():
            ctx.d2d(d_a, d_l, 32 * n)
            ctx.d2d(d_b, d_r, 32 * n)
            xl, xr, u = d_a, d_b, d_u
            for i in range(len(consts)):
                ctx.fr_vec_op(c, VEC_ADDC, xl, None, d_t, n, cw[i])
                ctx.fr_vec_op(c, VEC_MUL, d_t, d_t, u, n)
                ctx.fr_vec_op(c, VEC_MUL, u, d_t, u, n)
                ctx.fr_vec_op(c, VEC_ADD, u, xr, u, n)
                xl, xr, u = u, xl, xr
            ctx.sync()
            return xl
        fused()
        res = composed()
        a, b = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
        ctx.d2h(a, d_o)
        ctx.d2h(b, res)
        med = timed(ctx, {"fused": fused, "composed": composed, "composed_again": composed}, reps)
    finally:
        ctx.dev_free(d_a)
        ctx.dev_free(d_b)
    spread = abs(med["composed"] - med["composed_again"])
    comp = min(med["composed"], med["composed_again"])
    verdict = "within spread" if abs(med["fused"] - comp) <= spread else ("faster" if med["fused"] < comp else "slower")
    return dict(case="mimc_vs_composition", curve=c.name, hash=name, n=n, reps=reps, same_words=bool(np.array_equal(a, b)),
                launches=dict(fused=1, composed=4 * len(consts) + 2), fused_ms=round(med["fused"], 4), composed_ms=round(med["composed"], 4),
                composed_again_ms=round(med["composed_again"], 4), spread_ms=round(spread, 4),
                composed_over_fused=round(comp / med["fused"], 2), verdict=verdict)


def tree_case(ctx, c, hp, log, reps, d_nodes):
    n = 1 << log

    def run():
        ctx.fr_merkle_tree_dev(hp.handle, merkle.MERGE_BLOCK, d_nodes, n)
        ctx.sync()

    def tail():                                                   # 512 leaves: the tail launch and nothing else
        ctx.fr_merkle_tree_dev(hp.handle, merkle.MERGE_BLOCK, d_nodes, 512)
        ctx.sync()
    run()
    tail()
    med = timed(ctx, {"tree": run, "tail": tail}, reps)
    products = hp.info()["products"]
    return dict(case="tree", curve=c.name, hash="poseidon91", merge="block", n=n, reps=reps, launches=len(merkle.launch_plan(n)),
                ms=round(med["tree"], 4), tail_ms=round(med["tail"], 4), tail_share=round(med["tail"] / med["tree"], 3),
                tail_depths=hashes.HASH_TAIL_DEPTHS, gproducts_per_s=round((n - 1) * products / (med["tree"] * 1e-3) / 1e9, 2))


def witness_case(ctx, c, reps):
    S = samples_for_domain(20)
    t0 = time.perf_counter()
    inst = mimc_chain_instance(c, S)
    host_loop_s = time.perf_counter() - t0                        # the CSR arrays are built too: see csr_only_s
    t0 = time.perf_counter()
    mimc_chain_instance(c, S, with_witness=False)
    csr_only_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    z = codec.fr_to_mont(inst.z, c)
    encode_s = time.perf_counter() - t0
    hp = hashes.HashParams.mimc(ctx, c, inst.constants)
    pre = codec.fr_to_mont([a for a, _ in inst.preimages] + [b for _, b in inst.preimages], c)
    d_pre, d_z = ctx.to_device(pre), ctx.dev_alloc(z.nbytes)
    ptrs = []
    try:
        def upload():
            ctx.h2d(d_z, z)
            ctx.sync()

        def device():
            ptrs.append(hashes.mimc_chain_witness_dev(ctx, hp, d_pre, S))
            ctx.sync()
        upload()
        device()
        got = np.zeros_like(z)
        ctx.d2h(got, ptrs[-1])
        med = timed(ctx, {"upload": upload, "device": device}, reps)
    finally:
        for p in ptrs + [d_pre, d_z]:
            ctx.dev_free(p)
        hp.free()
    return dict(case="witness", curve=c.name, samples=S, elements=int(z.shape[0]), z_bytes=int(z.nbytes), reps=reps,
                same_words=bool(np.array_equal(got, z)), host_instance_s=round(host_loop_s, 2), host_csr_only_s=round(csr_only_s, 2),
                host_witness_loop_s=round(host_loop_s - csr_only_s, 2), host_encode_s=round(encode_s, 2),
                upload_ms=round(med["upload"], 3), device_ms=round(med["device"], 3),
                note="device_ms: allocation of z, the 32-byte copy of the constant one, one launch; the pre-images are resident")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--logs", type=int, nargs="*", default=[10, 14, 18, 20])
    ap.add_argument("--tree-logs", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--curves", nargs="*", default=["bn254", "bls12_381"])
    ap.add_argument("--only-tree", type=int, default=0)
    ap.add_argument("--witness-curves", nargs="*", default=["bn254"])
    args = ap.parse_args()
    ctx = Context(0)                                               # no GPU: this raises
    reps = max(args.reps, 3)
    for name in args.curves:
        c = get_curve(name)
        params, v = make_params(ctx, c)
        n_max = 1 << max(args.logs + args.tree_logs + [args.only_tree, 10])
        rng = np.random.default_rng(7)
        bufs = [ctx.to_device(rand_fr(rng, c, n_max)), ctx.to_device(rand_fr(rng, c, n_max))] + [ctx.dev_alloc(32 * n_max) for _ in range(3)]
        d_l, d_r, d_o, d_t, d_u = bufs
        d_nodes = ctx.to_device(rand_fr(rng, c, 2 * n_max - 1))
        try:
            if args.only_tree:
                for _ in range(3):
                    ctx.fr_merkle_tree_dev(params["poseidon91"].handle, merkle.MERGE_BLOCK, d_nodes, 1 << args.only_tree)
                ctx.sync()
                continue
            fr_rate = ctx.bench_mulmod(c, 0, False)
            for hname, hp in params.items():
                for log in args.logs:
                    print(json.dumps(blocks_case(ctx, c, hname, hp, log, reps, fr_rate, d_l, d_r, d_o)), flush=True)
            for hname, k in (("mimc5", 5), ("mimc322", 322)):
                for log in args.logs:
                    print(json.dumps(composition_case(ctx, c, hname, params[hname], v[:k], log, reps, d_l, d_r, d_o, d_t, d_u)), flush=True)
            for log in args.tree_logs:
                print(json.dumps(tree_case(ctx, c, params["poseidon91"], log, reps, d_nodes)), flush=True)
        finally:
            ctx.sync()
            for p in bufs + [d_nodes]:
                ctx.dev_free(p)
            for hp in params.values():
                hp.free()
        if name in args.witness_curves and not args.only_tree:
            print(json.dumps(witness_case(ctx, c, reps)), flush=True)


if __name__ == "__main__":
    assert MIMC_ROUNDS == 5
    main()
