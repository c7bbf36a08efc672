"""CPU: the bit gadgets (bits.py), the sha256 gadget, the membership gadget and the witness plan, on BLS12-381 and BN254.

The pins are the three numbers that the reference's own tests assert (tests/golden/sha256_reference.json), hashlib for every
digest, and the counts of a constant-propagating model of the gadget: 25 814 auxiliary variables beyond a block's 512 bits, and
44 874 constraints / 44 828 auxiliary variables for an allocated 64-byte message.  Each circuit is synthesised once per module."""
import functools
import hashlib
import itertools
import json
import random
from pathlib import Path

import pytest

from ckb_zkp_amd import circuits, merkle
from ckb_zkp_amd import sha256 as S
from ckb_zkp_amd.bits import CODE_ONE, AllocatedBit, Boolean, MultiEq, TaggedConstraintSystem, UInt32, code
from ckb_zkp_amd.r1cs import ConstraintSystem
from tests import sha256_ref as ref

CURVES = ["bls12_381", "bn254"]
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "sha256_reference.json").read_text())
LENGTHS = [0, 1, 31, 32, 55, 56, 64]
SEVEN = [bytes([i + 1]) * 32 for i in range(7)]                    # the example's leaves, one short of its eight


def rnd_bytes(seed, n):
    return bytes(random.Random(seed).getrandbits(8) for _ in range(n))


@functools.lru_cache(maxsize=None)
def block(curve, assign=True):
    bits = [random.Random(512).getrandbits(1) for _ in range(512)] if assign else None
    c = circuits.Sha256Block(bits)
    return (c,) + S.synthesize(c, curve, assign)


@functools.lru_cache(maxsize=None)
def message(curve, length, assign=True):
    c = ref.MessageCircuit(rnd_bytes(length, length)) if assign else ref.MessageCircuit(None, length)
    return (c,) + S.synthesize(c, curve, assign)


@functools.lru_cache(maxsize=None)
def membership(curve, n_leaves, leaf_index, assign=True):
    leaves = SEVEN if n_leaves == 7 else [rnd_bytes(100 * n_leaves + i, 32) for i in range(n_leaves)]
    nodes = ref.cbmt(leaves)
    lemmas = ref.cbmt_proof(nodes, leaf_index)
    index = n_leaves - 1 + leaf_index
    c = circuits.Sha256Merkle(index, leaves[leaf_index], lemmas, nodes[0]) if assign else \
        circuits.Sha256Merkle(index, None, [None] * len(lemmas), None)
    c.case = (index, leaves[leaf_index], lemmas, nodes[0])
    return (c,) + S.synthesize(c, curve, assign)


@pytest.mark.parametrize("curve", CURVES)
def test_blank_block_costs_nothing_and_gives_the_golden_digest(curve):
    cs = TaggedConstraintSystem(curve, True)
    bits = [Boolean.constant(i == 0) for i in range(512)]
    out = S.sha256_compression_function(cs, bits, S.get_sha256_iv(), 1)
    assert cs.num_constraints() == GOLDEN["blank_block_constraints"]["value"] == 0 and cs.num_aux == 0
    digest = [b for w in out for b in w.into_bits_be()]
    assert all(b.is_constant() for b in digest)
    assert ref.bits_to_bytes([b.get_value() for b in digest]).hex() == GOLDEN["blank_block_digest"]["value"]
    assert bytes.fromhex(GOLDEN["blank_block_digest"]["value"]) == hashlib.sha256(b"").digest()


@pytest.mark.parametrize("curve", CURVES)
def test_full_block_counts_and_is_satisfied(curve):
    c, cs, plan = block(curve)
    assert cs.num_constraints() - 512 == GOLDEN["full_block_constraints"]["value"] == 25840
    assert cs.num_aux - 512 == 25814 and cs.num_inputs == 1
    assert ref.is_satisfied(cs)
    # the first block of the message's hash, from the IV: the state after it, in the trace's final words
    t = ref.trace_one(c.message_bytes()[0])
    want = b"".join(t[1 + S.OFF_FINAL + 2 * k].to_bytes(4, "big") for k in range(8))
    assert ref.bits_to_bytes([b.get_value() for b in c.output]) == want


@pytest.mark.parametrize("curve", CURVES)
def test_a_flipped_witness_bit_is_not_satisfied(curve):
    _, cs, _ = block(curve)
    z = cs.full_assignment()
    for j in (1, 512, 513, len(z) - 1):                            # an input bit, the last input bit, a computed bit, the last bit
        bad = list(z)
        bad[j] ^= 1
        assert not ref.is_satisfied(cs, bad), j


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("curve", CURVES)
def test_sha256_of_allocated_messages(curve, length):
    c, cs, _ = message(curve, length)
    assert ref.is_satisfied(cs)
    want = S.bytes_to_bits(hashlib.sha256(c.data).digest())
    assert len(c.output) == 256
    for b, w in zip(c.output, want):                               # through Is / Not: the variable's value, complemented under Not
        assert b.get_value() == w
        if not b.is_constant():
            assert cs.full_assignment()[b.bit.variable[1] + cs.num_inputs] == (w if b.kind == 0 else 1 - w)
    if length == 64:
        assert cs.num_constraints() - 512 == 44874 and cs.num_aux - 512 == 44828
    if length == 0:
        assert cs.num_constraints() == 0 and cs.num_aux == 0      # everything is constant


@pytest.mark.parametrize("curve", CURVES)
def test_allocated_bit_truth_tables(curve):
    ops = {"xor": lambda x, y: x ^ y, "and_": lambda x, y: x & y, "and_not": lambda x, y: x & (1 - y), "nor": lambda x, y: (1 - x) & (1 - y)}
    for name, fn in ops.items():
        for x, y in itertools.product((0, 1), repeat=2):
            cs = ConstraintSystem(curve, True)
            a, b = AllocatedBit.alloc(cs, bool(x)), AllocatedBit.alloc(cs, bool(y))
            out = getattr(AllocatedBit, name)(cs, a, b)
            assert out.value == bool(fn(x, y)) and cs.num_constraints() == 3 and cs.num_aux == 3
            assert cs.aux_assignment == [x, y, fn(x, y)] and ref.is_satisfied(cs)
            assert not ref.is_satisfied(cs, [1, x, y, 1 - fn(x, y)]), (name, x, y)
    cs = ConstraintSystem(curve, True)
    AllocatedBit.alloc_input(cs, True)
    assert cs.num_inputs == 2 and not ref.is_satisfied(cs, [1, 2])                         # booleanity


def operand(cs, kind):
    """(Boolean, value) of one of the six operand kinds"""
    if kind in ("F", "T"):
        return Boolean.constant(kind == "T"), kind == "T"
    held = kind in ("is1", "not1")                                                         # the variable's value
    b = Boolean.is_(AllocatedBit.alloc(cs, held))
    return (b, held) if kind.startswith("is") else (b.not_(), not held)


def and_allocations(x, y):
    if "F" in (x, y):
        return 0
    return 0 if "T" in (x, y) else 1


def expected_allocations(fn, ka, kb, kc):
    """the folding arms of boolean.rs:481-543 / :588-646 in their match order -> variables allocated"""
    consts = sum(k in "FT" for k in (ka, kb, kc))
    if consts == 3:
        return 0
    if fn == "ch":
        if ka == "F":
            return 0
        if kb == "F" or kb == "T" and kc not in "FT":
            return and_allocations(ka, kc)
        if kc in "FT":
            return and_allocations(ka, kb)
        return 1
    if ka == "F":
        return and_allocations(kb, kc)
    if kb == "F":
        return and_allocations(ka, kc)
    if kc in "FT":
        return and_allocations(ka, kb)
    if kb == "T":
        return and_allocations(ka, kc)
    if ka == "T":
        return and_allocations(kb, kc)
    return 2


@pytest.mark.parametrize("fn", ["ch", "maj"])
@pytest.mark.parametrize("curve", CURVES)
def test_every_folding_arm_of_ch_and_maj(curve, fn):
    kinds = ["F", "T", "is0", "is1", "not0", "not1"]
    for ka, kb, kc in itertools.product(kinds, repeat=3):
        cs = TaggedConstraintSystem(curve, True)
        (a, va), (b, vb), (c, vc) = operand(cs, ka), operand(cs, kb), operand(cs, kc)
        before = cs.num_aux
        if fn == "ch":
            out, want = Boolean.sha256_ch(cs, a, b, c, (7, 3)), (va and vb) != ((not va) and vc)
        else:
            out, want = Boolean.sha256_maj(cs, a, b, c, (7, 3), (9, 3)), (va and vb) != ((va and vc) != (vb and vc))
        case = (fn, ka, kb, kc)
        assert out.get_value() == want, case
        assert cs.num_aux - before == expected_allocations(fn, ka, kb, kc), case
        assert ref.is_satisfied(cs), case
        new = cs.aux_tags[before:]
        if new:                                                    # the result's variable sits at (7, 3), complemented under Not
            assert not out.is_constant() and out.where() == code(7, 3), case
            assert new[0] == code(7, 3, 1 if out.kind == 1 else 0), case
            assert new[1:] in ([], [code(9, 3)]), case             # maj's internal b and c
            for t, v in zip(new, cs.aux_assignment[before:]):      # every tag agrees with the value: bit ^ neg
                bit = want if t >> 6 == 7 else (vb and vc)
                assert v == int(bit) ^ (t & 1), case


@pytest.mark.parametrize("curve", CURVES)
def test_addmany(curve):
    rng = random.Random(32)
    vals = [rng.getrandbits(32) for _ in range(10)] + [0xFFFFFFFF] * 10
    # constants only: a constant, nothing allocated, nothing pending
    cs = TaggedConstraintSystem(curve, True)
    with MultiEq(cs) as meq:
        out = UInt32.addmany(meq, [UInt32.constant(v) for v in vals[:3]])
    assert out.value == sum(vals[:3]) & 0xFFFFFFFF and all(b.is_constant() for b in out.bits)
    assert cs.num_aux == 0 and cs.num_constraints() == 0
    # mixed, and 10 operands at their largest: the result has the bits of the full integer sum
    for operands in (vals[:2], vals[3:8], vals[:10], vals[10:]):
        k = len(operands)
        cs = TaggedConstraintSystem(curve, True)
        with MultiEq(cs) as meq:
            ops = [UInt32.constant(v) if i % 2 else UInt32.alloc(cs, v, 40 + i) for i, v in enumerate(operands)]
            before = cs.num_aux
            out = UInt32.addmany(meq, ops, 5)
            assert cs.num_constraints() == before + (k * 0xFFFFFFFF).bit_length()          # booleanity only: the equality is pending
        nbits = (k * 0xFFFFFFFF).bit_length()
        assert nbits == {2: 33, 5: 35, 10: 36}[k] and cs.num_aux - before == nbits
        assert cs.num_constraints() == before + nbits + 1 and ref.is_satisfied(cs)
        total = sum(operands)
        assert out.value == total & 0xFFFFFFFF and len(out.bits) == 32
        assert cs.aux_assignment[before:] == [(total >> i) & 1 for i in range(nbits)]
        assert cs.aux_tags[before:] == [code(5 + i // 32, i % 32) for i in range(nbits)]
        bad = cs.full_assignment()
        bad[1 + before + 32] ^= 1                                                          # a carry bit
        assert not ref.is_satisfied(cs, bad)


@pytest.mark.parametrize("curve", CURVES)
def test_multieq_packs_until_the_capacity(curve):
    cs = TaggedConstraintSystem(curve, True)
    capacity = {"bls12_381": 254, "bn254": 253}[curve]
    meq = MultiEq(cs)
    assert meq.capacity == capacity
    x = UInt32.alloc(cs, 5, 2)
    lc = [t for i, b in enumerate(x.bits) for t in b.lc(1 << i)]
    fits = (capacity - 1) // 32
    for _ in range(fits):
        meq.enforce_equal(32, lc, lc)
    assert cs.num_constraints() == 32
    meq.enforce_equal(32, lc, lc)                                  # no room left: the pending constraint is emitted first
    assert cs.num_constraints() == 33
    meq.close()
    assert cs.num_constraints() == 34 and ref.is_satisfied(cs)


@pytest.mark.parametrize("leaf_index", [0, 1])
@pytest.mark.parametrize("curve", CURVES)
def test_membership_depth_two_left_and_right(curve, leaf_index):
    c, cs, _ = membership(curve, 4, leaf_index)
    index, leaf, lemmas, root = c.case
    assert len(lemmas) == 2 and (index & 1 == 1) == (leaf_index == 0)
    assert ref.cbmt_root(index, leaf, lemmas) == root
    assert cs.num_inputs == 257 and ref.is_satisfied(cs)
    bad = cs.full_assignment()
    bad[1] ^= 1                                                    # another root
    assert not ref.is_satisfied(cs, bad)


@pytest.mark.parametrize("leaf_index", range(7))
@pytest.mark.parametrize("curve", CURVES)
def test_membership_in_the_seven_leaf_tree(curve, leaf_index):
    c, cs, _ = membership(curve, 7, leaf_index)
    index, leaf, lemmas, root = c.case
    assert len(lemmas) == merkle.depth(index) and ref.cbmt_root(index, leaf, lemmas) == root
    assert ref.is_satisfied(cs)


def plan_cases(curve):
    b, m = block(curve), message(curve, 64)
    yield "block", b, b[0].message_bytes(), lambda: block(curve, False)
    yield "message", m, [m[0].data], lambda: message(curve, 64, False)
    for leaf_index in (0, 1):
        c = membership(curve, 4, leaf_index)
        index, leaf, lemmas, _ = c[0].case
        yield f"merkle{leaf_index}", c, merkle.membership_messages(index, leaf, lemmas), (lambda li=leaf_index: membership(curve, 4, li, False))


@pytest.mark.parametrize("curve", CURVES)
def test_the_plan_applied_to_the_reference_trace_is_the_assignment(curve):
    for name, (c, cs, plan), msgs, blank in plan_cases(curve):
        assert len(msgs) == plan.messages == c.messages and all(len(x) == plan.message_len for x in msgs), name
        assert len(plan.codes) == cs.num_inputs + cs.num_aux and plan.codes[0] == CODE_ONE, name
        assert None not in cs.tags(), name
        z = plan.apply(ref.trace(msgs))
        assert z == cs.full_assignment(), name
        # synthesis without values yields the same plan and the same shape
        _, cs0, plan0 = blank()
        assert plan0 == plan and (cs0.num_inputs, cs0.num_aux, cs0.num_constraints()) == (cs.num_inputs, cs.num_aux, cs.num_constraints()), name
        assert cs0.full_assignment() == [], name


def test_membership_messages_chain_to_the_root():
    nodes = ref.cbmt(SEVEN)
    for li in range(7):
        lemmas = ref.cbmt_proof(nodes, li)
        msgs = merkle.membership_messages(6 + li, SEVEN[li], lemmas)
        assert len(msgs) == len(lemmas) and all(len(x) == 64 for x in msgs)
        assert hashlib.sha256(msgs[-1]).digest() == nodes[0]
        assert SEVEN[li] in (msgs[0][:32], msgs[0][32:])
