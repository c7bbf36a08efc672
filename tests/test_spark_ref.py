"""CPU: tests/spark_ref.py against the plain product, a hand-computed circuit, the layer layout of the device buffers, the
memory-checking identity and the verifier of the product-circuit proof."""
import hashlib
import random

import pytest

from tests import spark_ref as ref

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617      # BN254 Fr


def _callbacks(tag=b""):
    """deterministic stand-ins for the transcript: a counter plus whatever the reference would have absorbed"""
    state = {"n": 0}

    def h(*parts):
        state["n"] += 1
        data = tag + state["n"].to_bytes(4, "little") + b"".join(int(v).to_bytes(32, "little") for v in parts)
        return int.from_bytes(hashlib.sha256(data).digest(), "little") % R

    def next_coeffs(count):
        return [h(count, i) for i in range(count)]

    def next_round(coeffs):
        return h(*coeffs)

    def next_layer(left, right, dotp):
        return h(*left, *right, *([v for t in dotp for v in t] if dotp else []))

    return next_coeffs, next_round, next_layer


def test_root_is_the_plain_product():
    rnd = random.Random(1)
    for n in (2, 4, 8, 64, 256):
        vals = [rnd.randrange(R) for _ in range(n)]
        circ = ref.construct_product_circuit(vals, R)
        prod = 1
        for v in vals:
            prod = prod * v % R
        assert ref.evaluate_product_circuit(circ, R) == prod
        assert len(circ[0]) == n.bit_length() - 1 and len(ref.flatten(circ)) == 2 * n - 2


def test_hand_computed_four_leaves():
    left, right = ref.construct_product_circuit([2, 3, 5, 7], R)
    assert left == [[2, 3], [10]] and right == [[5, 7], [21]]
    assert ref.flatten((left, right)) == [2, 3, 5, 7, 10, 21]
    assert ref.evaluate_product_circuit((left, right), R) == 210
    assert ref.circuit_hash([3], [5], [7], 2, R) == [3 * 4 + 5 * 2 + 7]


def test_layer_offsets_and_strided_products():
    rnd = random.Random(2)
    n = 64
    vals = [rnd.randrange(R) for _ in range(n)]
    circ = ref.construct_product_circuit(vals, R)
    flat = ref.flatten(circ)
    assert [ref.layer_offset(8, l) for l in range(3)] == [0, 8, 12]
    for l in range(6):
        off, ln = ref.layer_offset(n, l), n >> l
        assert flat[off:off + ln] == circ[0][l] + circ[1][l]
        assert ref.layer_offset(n, l + 1) == off + ln
    assert ref.layer_offset(n, 6) == 2 * n - 2
    # layer[l + k][j] is the product of the 2^k elements layer[l][j + s (len >> k)]
    layer = lambda l: flat[ref.layer_offset(n, l):ref.layer_offset(n, l + 1)]            # noqa: E731
    for l, k in ((0, 3), (1, 2), (2, 3), (0, 1)):
        src, dst = layer(l), layer(l + k)
        step = len(src) >> k
        for j in range(step):
            prod = 1
            for s in range(1 << k):
                prod = prod * src[j + s * step] % R
            assert dst[j] == prod


def _instance(seed, k, n, m):
    rnd = random.Random(seed)
    addrs_list = [[rnd.randrange(m) for _ in range(n)] for _ in range(k)]
    addrs_list[0][0], addrs_list[-1][-1] = m - 1, 0
    mem = [rnd.randrange(R) for _ in range(m)]
    e_list = [[mem[a] for a in addrs] for addrs in addrs_list]
    read_ts, audit_ts = ref.memory_in_the_head(addrs_list, m)
    gamma = (rnd.randrange(R), rnd.randrange(R))
    return addrs_list, mem, read_ts, audit_ts, e_list, gamma


@pytest.mark.parametrize("n,m", [(16, 4), (8, 8), (8, 64)])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_memory_checking_identity(k, n, m):
    addrs_list, mem, read_ts, audit_ts, e_list, gamma = _instance(10 * k + n, k, n, m)
    assert sum(audit_ts) == k * n and max(max(t) for t in read_ts) < k * n
    layer = ref.memory_checking(addrs_list, mem, read_ts, audit_ts, e_list, gamma, R)
    assert len(layer["read"]) == len(layer["write"]) == k
    assert len(layer["init"][0]) == m.bit_length() - 1 and len(layer["read"][0][0]) == n.bit_length() - 1
    # leaf 0 of the first read circuit, spelled out
    g1, g2 = gamma
    assert layer["read"][0][0][0][0] == (addrs_list[0][0] * g1 * g1 + e_list[0][0] * g1 + read_ts[0][0] - g2) % R
    assert layer["write"][0][0][0][0] == (layer["read"][0][0][0][0] + 1) % R
    bad = [list(e) for e in e_list]
    bad[-1][3] = (bad[-1][3] + 1) % R
    with pytest.raises(AssertionError):
        ref.memory_checking(addrs_list, mem, read_ts, audit_ts, bad, gamma, R)


@pytest.mark.parametrize("with_dotp", [False, True])
def test_verifier_accepts_the_prover_and_rejects_a_changed_coefficient(with_dotp):
    k, n, m = 2, 16, 4
    addrs_list, mem, read_ts, audit_ts, e_list, gamma = _instance(7, k, n, m)
    layer = ref.memory_checking(addrs_list, mem, read_ts, audit_ts, e_list, gamma, R)
    circuits = [c for pair in zip(layer["read"], layer["write"]) for c in pair]
    rnd = random.Random(8)
    dotp = []
    if with_dotp:
        full = [[rnd.randrange(R) for _ in range(n)] for _ in range(3)]
        dotp = [tuple(t[:n // 2] for t in full), tuple(t[n // 2:] for t in full)]
    layers, claim_dotp, rands = ref.product_circuit_eval_prover(circuits, dotp, *_callbacks(), R)
    assert len(layers) == 4 and [len(p) for p, _, _ in layers] == [0, 1, 2, 3] and len(rands) == 4
    roots = [ref.evaluate_product_circuit(c, R) for c in circuits]
    sums = [ref.evaluate_dot_product_circuit(*t, R) for t in dotp]
    claims, claims_dotp, v_rands = ref.product_circuit_eval_verify((layers, claim_dotp), roots, sums, n, *_callbacks(), R)
    assert v_rands == rands and len(claims) == len(circuits) and len(claims_dotp) == (3 if with_dotp else 0)
    # the claims that remain are the leaves' multilinear extensions at rands
    eq = ref.eval_eq(rands, R)
    for c, claim in zip(circuits, claims):
        assert claim == sum(e * v for e, v in zip(eq, c[0][0] + c[1][0])) % R
    if with_dotp:
        assert claims_dotp == [sum(e * v for e, v in zip(eq, t)) % R for t in full]
    polys, left, right = layers[-1]
    tampered = layers[:-1] + [([list(polys[0][:1]) + [(polys[0][1] + 1) % R] + list(polys[0][2:])] + polys[1:], left, right)]
    with pytest.raises(AssertionError):
        ref.product_circuit_eval_verify((tampered, claim_dotp), roots, sums, n, *_callbacks(), R)
    with pytest.raises(AssertionError):
        ref.product_circuit_eval_verify((layers, claim_dotp), [(roots[0] + 1) % R] + roots[1:], sums, n, *_callbacks(), R)
