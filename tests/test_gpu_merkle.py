"""zkp_fr_merkle_tree_dev / zkp_fr_merkle_paths_dev and ckb_zkp_amd.merkle on the device, bit-exact against the CBMT of
tests/hash_ref.py.  The node buffer is framed by sentinels and compared whole; the leaves are read back unchanged as part of it.

Sizes: one leaf (no launch), the reference's 2 and 5, 3; 255 / 256 / 257 (depth 7 one node short of full, full, and with the
first node of depth 8); 511 / 512 (depth 8 one node short of full, then all 256 lanes of the tail busy) and 513 (depth 9 as a launch of ONE node);
1025 (two depth launches, the first of one node, plus the tail).  Wherever n is no power of two the leaves span two depths."""
import numpy as np
import pytest

from ckb_zkp_amd import _lib, codec, hashes, merkle
from ckb_zkp_amd.circuits import prf_field_elements
from ckb_zkp_amd.params import get_curve
from tests import hash_cases as cases
from tests import hash_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "bls12_381"]
SENT = 0xDEADBEEFCAFEF00D
NS = [1, 2, 3, 5, 255, 256, 257, 511, 512, 513, 1025]
MERGES = {merkle.MERGE_BLOCK: ref.merge_block, merkle.MERGE_CHAIN: ref.merge_chain}
_CACHE = {}


def hash_set(ctx, curve, kind):
    """(parameter dict, HashParams): MiMC-5 and a short Poseidon (2 full, 3 partial, 2 full), uploaded once"""
    key = (curve, kind)
    if key not in _CACHE:
        p = cases.mimc_params(curve, 5) if kind == "mimc" else cases.poseidon_params(curve, hashes.poseidon_schedule(2, 3, 2))
        _CACHE[key] = (p, cases.upload(ctx, curve, p))
    return _CACHE[key]


def reference_tree(curve, kind, merge, n, p):
    """the Python tree of one case, computed once and shared by the tree and the path tests"""
    key = (curve, kind, merge, n)
    if key not in _CACHE:
        leaves = prf_field_elements(0x7EE + n, n, p["r"])
        leaves[0], leaves[-1] = 0, p["r"] - 1
        _CACHE[key] = ref.build_tree(leaves, MERGES[merge](p))
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _free_sets():
    yield
    for v in _CACHE.values():
        if isinstance(v, tuple):
            v[1].free()
    _CACHE.clear()


def read(ctx, ptr, like):
    got = np.zeros_like(like)
    ctx.d2h(got, ptr)
    return got


def framed_tree(c, nodes, n):
    """sentinels, the inner nodes as sentinels, the leaves, sentinels"""
    host = np.full((2 * n + 1, 4), SENT, dtype=np.uint64)
    host[n:2 * n] = codec.fr_to_mont(nodes[n - 1:], c)
    return host


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("merge", list(MERGES))
@pytest.mark.parametrize("kind", ["mimc", "poseidon"])
@pytest.mark.parametrize("curve", CURVES)
def test_tree(ctx, curve, kind, merge, n):
    c = get_curve(curve)
    p, hp = hash_set(ctx, curve, kind)
    nodes = reference_tree(curve, kind, merge, n, p)
    if n & (n - 1):
        assert merkle.depth(n - 1) + 1 == merkle.depth(2 * n - 2)                 # the leaves span two depths
    host = framed_tree(c, nodes, n)
    d = ctx.to_device(host)
    try:
        ctx.fr_merkle_tree_dev(hp.handle, merge, d + 32, n)
        ctx.sync()
        got = read(ctx, d, host)
    finally:
        ctx.dev_free(d)
    want = host.copy()
    want[1:2 * n] = codec.fr_to_mont(nodes, c)
    assert np.array_equal(got, want), (curve, kind, merge, n)
    assert len(merkle.launch_plan(n)) == {1: 0, 513: 2, 1025: 3}.get(n, 1)
    if n in (5, 513):
        # the driver builds the same tree from integers, and the queue algorithm reaches the same root
        tree = merkle.build_tree(hp, nodes[n - 1:], merge)
        try:
            assert np.array_equal(tree.nodes(), want[1:2 * n]) and np.array_equal(merkle.root(tree), want[1])
        finally:
            tree.free()
        assert ref.build_merkle_root(nodes[n - 1:], MERGES[merge](p)) == nodes[0]


@pytest.mark.parametrize("n", [1, 5, 513])
@pytest.mark.parametrize("curve", CURVES)
def test_paths(ctx, curve, n):
    """every leaf, then repeats, an unsorted order and an index that is no leaf; the rows' tails; every path recomputes the root"""
    c = get_curve(curve)
    merge = merkle.MERGE_BLOCK
    p, hp = hash_set(ctx, curve, "mimc")
    nodes = reference_tree(curve, "mimc", merge, n, p)
    idx = list(range(n)) + [n - 1, 0, 0, n // 2, n, n + 7, 0xFFFFFFFF, n - 1]
    q = len(idx)
    for stride in (merkle.depth(2 * n - 2), merkle.depth(2 * n - 2) + 2):
        rows = max(q * stride, 1)
        h_n = np.concatenate([np.full((1, 4), SENT, dtype=np.uint64), codec.fr_to_mont(nodes, c), np.full((1, 4), SENT, dtype=np.uint64)])
        h_o = np.full((rows + 2, 4), SENT, dtype=np.uint64)
        h_l = np.full(q + 2, 0xABABABAB, dtype=np.uint32)
        h_i = np.array(idx, dtype=np.uint32)
        d_n, d_o, d_l, d_i = ctx.to_device(h_n), ctx.to_device(h_o), ctx.to_device(h_l), ctx.to_device(h_i)
        try:
            ctx.fr_merkle_paths_dev(d_n + 32, n, d_i, q, d_o + 32, stride, d_l + 4)
            ctx.sync()
            g_n, g_o, g_l, g_i = read(ctx, d_n, h_n), read(ctx, d_o, h_o), read(ctx, d_l, h_l), read(ctx, d_i, h_i)
        finally:
            for d in (d_n, d_o, d_l, d_i):
                ctx.dev_free(d)
        assert np.array_equal(g_n, h_n) and np.array_equal(g_i, h_i), "an input changed"
        want_o, want_l = h_o.copy(), h_l.copy()
        if stride:
            want_o[1:1 + q * stride] = 0
        for k, leaf in enumerate(idx):
            if leaf >= n:
                want_l[1 + k] = merkle.BAD_LEAF
                continue
            index, lemmas = ref.build_proof(nodes, leaf)
            assert len(lemmas) == merkle.depth(n - 1 + leaf) <= stride
            want_l[1 + k] = len(lemmas)
            if lemmas:
                want_o[1 + k * stride:1 + k * stride + len(lemmas)] = codec.fr_to_mont(lemmas, c)
            got_lemmas = codec.fr_from_mont(g_o[1 + k * stride:1 + k * stride + len(lemmas)], c) if lemmas else []
            assert ref.proof_root(index, got_lemmas, nodes[index], MERGES[merge](p)) == nodes[0], (n, leaf)
        assert np.array_equal(g_l, want_l)
        assert np.array_equal(g_o, want_o)
        lens = {int(v) for v in g_l[1:1 + n]}
        assert max(lens) - min(lens) <= 1                                          # the leaves sit on at most two depths


@pytest.mark.parametrize("curve", CURVES)
def test_driver_proofs(ctx, curve):
    c = get_curve(curve)
    p, hp = hash_set(ctx, curve, "poseidon")
    n = 10
    for merge in MERGES:
        nodes = reference_tree(curve, "poseidon", merge, n, p)
        tree = merkle.build_tree(hp, nodes[n - 1:], merge)
        try:
            order = [9, 0, 4, 4, 7]
            for leaf, lemmas in zip(order, merkle.build_proofs(tree, order)):
                index, want = ref.build_proof(nodes, leaf)
                assert codec.fr_from_mont(lemmas, c) == want if want else len(lemmas) == 0
                assert ref.proof_root(index, codec.fr_from_mont(lemmas, c), nodes[index], MERGES[merge](p)) == nodes[0]
            with pytest.raises(IndexError):
                merkle.build_proofs(tree, [3, n])
            assert merkle.build_proofs(tree, []) == []
        finally:
            tree.free()
    with pytest.raises(ValueError):
        merkle.build_tree(hp, [])


def _bad(fn, status=-1):
    with pytest.raises(_lib.ZkpError) as e:
        fn()
    assert e.value.status == status


@pytest.mark.parametrize("curve", CURVES)
def test_argument_rules(ctx, curve):
    _, hp = hash_set(ctx, curve, "mimc")
    n, q = 5, 3
    host = np.full((64, 4), SENT, dtype=np.uint64)
    d = ctx.to_device(host)
    nodes, out, idx, lens = d + 32, d + 32 * 16, d + 32 * 40, d + 32 * 48        # 9 nodes; 3 rows of 3; 3 indices; 3 lengths
    try:
        tree = lambda h=hp.handle, m=0, p=nodes, cnt=n: ctx.fr_merkle_tree_dev(h, m, p, cnt)                          # noqa: E731
        paths = lambda p=nodes, cnt=n, i=idx, k=q, o=out, st=3, ln=lens: ctx.fr_merkle_paths_dev(p, cnt, i, k, o, st, ln)   # noqa: E731
        _bad(lambda: tree(h=0))
        _bad(lambda: tree(p=0))
        _bad(lambda: tree(p=nodes + 8))
        _bad(lambda: tree(m=2))
        _bad(lambda: tree(m=-1))
        _bad(lambda: tree(cnt=0))
        _bad(lambda: tree(cnt=(1 << hashes.HASH_MAX_LOG_LEAVES) + 1))
        for kw in ({"p": 0}, {"i": 0}, {"o": 0}, {"ln": 0}):
            _bad(lambda: paths(**kw))
        for kw in ({"p": nodes + 8}, {"o": out + 8}, {"i": idx + 2}, {"ln": lens + 2}):
            _bad(lambda: paths(**kw))
        _bad(lambda: paths(cnt=0))
        _bad(lambda: paths(cnt=(1 << hashes.HASH_MAX_LOG_LEAVES) + 1, st=40))
        _bad(lambda: paths(k=0))
        _bad(lambda: paths(k=(1 << hashes.HASH_MAX_LOG_BLOCKS) + 1))
        _bad(lambda: paths(st=2))                                                      # depth(2 n - 2) = 3
        _bad(lambda: paths(k=1 << 20, st=(1 << 12) + 1))                               # q stride above 2^32
        _bad(lambda: paths(o=nodes + 32 * 8))                                          # the rows on the last node
        _bad(lambda: paths(o=idx - 32 * 9 + 32))                                       # the rows' last element on the indices
        _bad(lambda: paths(ln=out + 32 * 8))                                           # the lengths inside the rows
        _bad(lambda: paths(ln=idx + 8))                                                # the lengths on the indices
        _bad(lambda: paths(ln=nodes))                                                  # the lengths on the nodes
        ctx.sync()
        assert np.array_equal(read(ctx, d, host), host), "an output changed on an error"
        # n == 1: nothing to compute, nothing written; its one path is empty
        tree(cnt=1)
        ctx.sync()
        assert np.array_equal(read(ctx, d, host), host)
    finally:
        ctx.dev_free(d)
