"""The bit gadgets of the reference's gadgets package over r1cs.ConstraintSystem: AllocatedBit and Boolean
(gadgets/src/algebra/boolean.rs:9-305, :310-685), UInt32 (gadgets/src/algebra/uint32.rs:12-370) and MultiEq
(gadgets/src/operator/multieq.rs:6-66).  A restatement: same constraint shapes, same allocation order, same constant folding in the
same match order, because the order decides which variables exist.

What is added: every operation that may allocate a variable takes the place of its result in a word-major trace (sha256.py), and
the variable is tagged with the code `v << 6 | bit << 1 | neg` of that place.  `neg` says that the variable holds the complement of
the trace bit: the folded arms of sha256_ch / sha256_maj return Not(and(..)), and Is ^ Not allocates the XOR of the two variables.
A TaggedConstraintSystem keeps one code per variable; a plain ConstraintSystem ignores the tags."""
from __future__ import annotations

from .r1cs import INPUT, ConstraintSystem, LinearCombination

ONE = (INPUT, 0)
CODE_ZERO, CODE_ONE = 0, 1                 # word 0 of a trace is 0: bit 0 of it, plain and complemented
CODE_WORD_BITS = 26                        # ZKP_SHA256_MAX_LOG_CODE_WORDS


def code(v: int, bit: int, neg: int = 0) -> int:
    if not (0 <= v < 1 << CODE_WORD_BITS and 0 <= bit < 32):
        raise ValueError(f"no code for word {v}, bit {bit}")
    return v << 6 | bit << 1 | (neg & 1)


class TaggedConstraintSystem(ConstraintSystem):
    """A ConstraintSystem that keeps, for every variable, the code of the trace bit it holds (None: untagged)."""

    def __init__(self, curve, assign: bool):
        self.input_tags, self.aux_tags = [], []
        super().__init__(curve, assign)
        self.input_tags[0] = CODE_ONE

    def alloc(self, f, tag=None):
        self.aux_tags.append(tag)
        return super().alloc(f)

    def alloc_input(self, f, tag=None):
        self.input_tags.append(tag)
        return super().alloc_input(f)

    def tags(self) -> list:
        return self.input_tags + self.aux_tags


def alloc_tagged(cs, value, tag, public: bool = False):
    """one variable holding `value` (None: missing), tagged with the code `tag` where the system keeps tags"""
    fn = cs.alloc_input if public else cs.alloc
    f = (lambda: None) if value is None else (lambda: int(value))
    return fn(f, tag) if tag is not None and getattr(cs, "tagged", False) else fn(f)


TaggedConstraintSystem.tagged = True


def _lc(terms):
    return lambda _: LinearCombination(terms)


def _sub(a, b):
    return a + [(var, -coeff) for var, coeff in b]


def _tag(pos, neg):
    return None if pos is None else code(pos[0], pos[1], neg)


class AllocatedBit:
    """boolean.rs:9-305: a variable constrained to 0 or 1"""
    __slots__ = ("variable", "value", "tag")

    def __init__(self, variable, value, tag=None):
        self.variable, self.value, self.tag = variable, value, tag

    @classmethod
    def _boolean(cls, cs, value, tag, public):
        var = alloc_tagged(cs, value, tag, public)
        cs.enforce(_lc([(ONE, 1), (var, -1)]), _lc([(var, 1)]), _lc([]))                 # (1 - a) a = 0
        return cls(var, value, tag)

    @classmethod
    def alloc(cls, cs, value, tag=None):                                                  # :67-96
        return cls._boolean(cs, value, tag, False)

    @classmethod
    def alloc_input(cls, cs, value, tag=None):                                            # :100-129
        return cls._boolean(cs, value, tag, True)

    @classmethod
    def _binary(cls, cs, a, b, fn, tag, rows):
        value = None if a.value is None or b.value is None else bool(fn(a.value, b.value))
        var = alloc_tagged(cs, value, tag)
        ra, rb, rc = rows(var)
        cs.enforce(_lc(ra), _lc(rb), _lc(rc))
        return cls(var, value, tag)

    @classmethod
    def xor(cls, cs, a, b, tag=None):                                                     # :133-183: (a + a) b = a + b - c
        return cls._binary(cs, a, b, lambda x, y: x ^ y, tag, lambda c: (
            [(a.variable, 1), (a.variable, 1)], [(b.variable, 1)], [(a.variable, 1), (b.variable, 1), (c, -1)]))

    @classmethod
    def and_(cls, cs, a, b, tag=None):                                                    # :187-224: a b = c
        return cls._binary(cs, a, b, lambda x, y: x and y, tag, lambda c: ([(a.variable, 1)], [(b.variable, 1)], [(c, 1)]))

    @classmethod
    def and_not(cls, cs, a, b, tag=None):                                                 # :227-264: a (1 - b) = c
        return cls._binary(cs, a, b, lambda x, y: x and not y, tag, lambda c: (
            [(a.variable, 1)], [(ONE, 1), (b.variable, -1)], [(c, 1)]))

    @classmethod
    def nor(cls, cs, a, b, tag=None):                                                     # :267-304: (1 - a) (1 - b) = c
        return cls._binary(cs, a, b, lambda x, y: not x and not y, tag, lambda c: (
            [(ONE, 1), (a.variable, -1)], [(ONE, 1), (b.variable, -1)], [(c, 1)]))


IS, NOT, CONSTANT = 0, 1, 2


class Boolean:
    """boolean.rs:310-685: Is(bit), Not(bit) or Constant(bool).  The operations that may allocate take `pos`, the (word, bit) of
    their RESULT in the trace, and `neg`, whether the variable they allocate is to hold that bit's complement."""
    __slots__ = ("kind", "bit", "const")

    def __init__(self, kind, bit=None, const=False):
        self.kind, self.bit, self.const = kind, bit, bool(const)

    @classmethod
    def constant(cls, b) -> "Boolean":
        return cls(CONSTANT, None, b)

    @classmethod
    def is_(cls, bit: AllocatedBit) -> "Boolean":
        return cls(IS, bit)

    def is_constant(self) -> bool:
        return self.kind == CONSTANT

    def get_value(self):
        if self.kind == CONSTANT:
            return self.const
        v = self.bit.value
        return None if v is None else (bool(v) if self.kind == IS else not v)

    def where(self):
        """the code of the trace bit that equals this Boolean's value (None: an untagged variable)"""
        if self.kind == CONSTANT:
            return CODE_ONE if self.const else CODE_ZERO
        return None if self.bit.tag is None else self.bit.tag ^ (1 if self.kind == NOT else 0)

    def lc(self, coeff: int = 1) -> list:                                                 # :381-395, as (variable, coeff) terms
        if self.kind == CONSTANT:
            return [(ONE, coeff)] if self.const else []
        if self.kind == IS:
            return [(self.bit.variable, coeff)]
        return [(ONE, coeff), (self.bit.variable, -coeff)]

    def not_(self) -> "Boolean":                                                          # :403-409
        if self.kind == CONSTANT:
            return Boolean(CONSTANT, None, not self.const)
        return Boolean(NOT if self.kind == IS else IS, self.bit)

    @staticmethod
    def xor(cs, a, b, pos=None, neg=0) -> "Boolean":                                      # :412-431
        if a.kind == CONSTANT and not a.const:
            return b
        if b.kind == CONSTANT and not b.const:
            return a
        if a.kind == CONSTANT:
            return b.not_()
        if b.kind == CONSTANT:
            return a.not_()
        if a.kind != b.kind:                                                              # a ^ not b = not (a ^ b)
            is_, nt = (a, b) if a.kind == IS else (b, a)
            return Boolean.xor(cs, is_, nt.not_(), pos, neg ^ 1).not_()
        return Boolean.is_(AllocatedBit.xor(cs, a.bit, b.bit, _tag(pos, neg)))

    @staticmethod
    def and_(cs, a, b, pos=None, neg=0) -> "Boolean":                                     # :434-460
        if (a.kind == CONSTANT and not a.const) or (b.kind == CONSTANT and not b.const):
            return Boolean.constant(False)
        if a.kind == CONSTANT:
            return b
        if b.kind == CONSTANT:
            return a
        tag = _tag(pos, neg)
        if a.kind != b.kind:
            is_, nt = (a, b) if a.kind == IS else (b, a)
            return Boolean.is_(AllocatedBit.and_not(cs, is_.bit, nt.bit, tag))
        if a.kind == NOT:
            return Boolean.is_(AllocatedBit.nor(cs, a.bit, b.bit, tag))
        return Boolean.is_(AllocatedBit.and_(cs, a.bit, b.bit, tag))

    @staticmethod
    def sha256_ch(cs, a, b, c, pos=None) -> "Boolean":                                    # :463-567: (a and b) xor ((not a) and c)
        va, vb, vc = a.get_value(), b.get_value(), c.get_value()
        value = None if va is None or vb is None or vc is None else (va and vb) != ((not va) and vc)
        ka, kb, kc = a.kind == CONSTANT, b.kind == CONSTANT, c.kind == CONSTANT
        if ka and kb and kc:
            return Boolean.constant(value)
        if ka and not a.const:
            return c
        if kb and not b.const:
            return Boolean.and_(cs, a.not_(), c, pos)
        if kc and not c.const:
            return Boolean.and_(cs, a, b, pos)
        if kc:
            return Boolean.and_(cs, a, b.not_(), pos, 1).not_()
        if kb:
            return Boolean.and_(cs, a.not_(), c.not_(), pos, 1).not_()
        tag = _tag(pos, 0)
        ch = alloc_tagged(cs, value, tag)
        cs.enforce(_lc(_sub(b.lc(), c.lc())), _lc(a.lc()), _lc(_sub([(ch, 1)], c.lc())))   # a (b - c) = ch - c
        return Boolean.is_(AllocatedBit(ch, value, tag))

    @staticmethod
    def sha256_maj(cs, a, b, c, pos=None, pos_bc=None) -> "Boolean":                      # :570-684: (a and b) xor (a and c) xor (b and c)
        va, vb, vc = a.get_value(), b.get_value(), c.get_value()
        value = None if va is None or vb is None or vc is None else (va and vb) != ((va and vc) != (vb and vc))
        ka, kb, kc = a.kind == CONSTANT, b.kind == CONSTANT, c.kind == CONSTANT
        if ka and kb and kc:
            return Boolean.constant(value)
        if ka and not a.const:
            return Boolean.and_(cs, b, c, pos)
        if kb and not b.const:
            return Boolean.and_(cs, a, c, pos)
        if kc and not c.const:
            return Boolean.and_(cs, a, b, pos)
        if kc:
            return Boolean.and_(cs, a.not_(), b.not_(), pos, 1).not_()
        if kb:
            return Boolean.and_(cs, a.not_(), c.not_(), pos, 1).not_()
        if ka:
            return Boolean.and_(cs, b.not_(), c.not_(), pos, 1).not_()
        tag = _tag(pos, 0)
        maj = alloc_tagged(cs, value, tag)
        bc = Boolean.and_(cs, b, c, pos_bc)
        # (2 bc - b - c) a = bc - maj
        cs.enforce(_lc(_sub(_sub(bc.lc() + bc.lc(), b.lc()), c.lc())), _lc(a.lc()), _lc(_sub(bc.lc(), [(maj, 1)])))
        return Boolean.is_(AllocatedBit(maj, value, tag))


class MultiEq:
    """multieq.rs:6-66: packs equalities of few bits into one constraint until the field's CAPACITY is reached.  It stands in for
    the system it wraps; close() (or leaving the `with` block) emits what is pending, where Rust drops the object."""

    def __init__(self, cs):
        self.cs = cs
        self.capacity = cs.curve.r.bit_length() - 1
        self.ops = self.bits_used = 0
        self.lhs, self.rhs = [], []

    def __getattr__(self, name):
        return getattr(self.cs, name)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.close()
        return False

    def _accumulate(self):
        self.cs.enforce(_lc(self.lhs), _lc([(ONE, 1)]), _lc(self.rhs))
        self.lhs, self.rhs, self.bits_used = [], [], 0
        self.ops += 1

    def enforce_equal(self, num_bits: int, lhs: list, rhs: list):
        if self.capacity <= self.bits_used + num_bits:
            self._accumulate()
        assert self.capacity > self.bits_used + num_bits
        shift = 1 << self.bits_used
        self.lhs = self.lhs + [(var, coeff * shift) for var, coeff in lhs]
        self.rhs = self.rhs + [(var, coeff * shift) for var, coeff in rhs]
        self.bits_used += num_bits

    def close(self):
        if self.bits_used > 0:
            self._accumulate()


class UInt32:
    """uint32.rs:12-370: 32 Booleans, least significant first.  `word`: the index of the result's word in the trace (a sum: its
    low word, the high word follows)."""
    __slots__ = ("bits", "value")

    def __init__(self, bits, value):
        self.bits, self.value = bits, value

    @classmethod
    def constant(cls, value: int) -> "UInt32":
        return cls([Boolean.constant((value >> i) & 1) for i in range(32)], value & 0xFFFFFFFF)

    @classmethod
    def alloc(cls, cs, value, word=None) -> "UInt32":
        bits = [Boolean.is_(AllocatedBit.alloc(cs, None if value is None else bool((value >> i) & 1),
                                                None if word is None else code(word, i))) for i in range(32)]
        return cls(bits, value)

    @classmethod
    def from_bits_be(cls, bits) -> "UInt32":
        assert len(bits) == 32
        value = 0
        for b in bits:
            v = b.get_value()
            value = None if value is None or v is None else value << 1 | int(v)
        return cls(list(reversed(bits)), value)

    def into_bits_be(self) -> list:
        return list(reversed(self.bits))

    def rotr(self, by: int) -> "UInt32":
        by %= 32
        v = self.value
        return UInt32(self.bits[by:] + self.bits[:by], None if v is None else (v >> by | v << (32 - by)) & 0xFFFFFFFF)

    def shr(self, by: int) -> "UInt32":
        by %= 32
        return UInt32(self.bits[by:] + [Boolean.constant(False)] * by, None if self.value is None else self.value >> by)

    def xor(self, cs, other, word=None) -> "UInt32":
        value = None if self.value is None or other.value is None else self.value ^ other.value
        return UInt32([Boolean.xor(cs, a, b, None if word is None else (word, i))
                       for i, (a, b) in enumerate(zip(self.bits, other.bits))], value)

    @staticmethod
    def sha256_ch(cs, a, b, c, word=None) -> "UInt32":
        value = None if None in (a.value, b.value, c.value) else (a.value & b.value) ^ (~a.value & c.value & 0xFFFFFFFF)
        return UInt32([Boolean.sha256_ch(cs, x, y, z, None if word is None else (word, i))
                       for i, (x, y, z) in enumerate(zip(a.bits, b.bits, c.bits))], value)

    @staticmethod
    def sha256_maj(cs, a, b, c, word=None, word_bc=None) -> "UInt32":
        value = None if None in (a.value, b.value, c.value) else (a.value & b.value) ^ (a.value & c.value) ^ (b.value & c.value)
        return UInt32([Boolean.sha256_maj(cs, x, y, z, None if word is None else (word, i), None if word_bc is None else (word_bc, i))
                       for i, (x, y, z) in enumerate(zip(a.bits, b.bits, c.bits))], value)

    @staticmethod
    def addmany(cs: MultiEq, operands, word=None) -> "UInt32":                            # :271-369
        assert 2 <= len(operands) <= 10
        max_value = len(operands) * 0xFFFFFFFF
        result_value, lc, all_constants = 0, [], True
        for op in operands:
            result_value = None if result_value is None or op.value is None else result_value + op.value
            for i, bit in enumerate(op.bits):
                lc += bit.lc(1 << i)
                all_constants = all_constants and bit.is_constant()
        if all_constants and result_value is not None:
            return UInt32.constant(result_value & 0xFFFFFFFF)
        bits, result_lc = [], []
        nbits = max_value.bit_length()                      # the bits of the full integer sum, carries included
        for i in range(nbits):
            tag = None if word is None else code(word + (i >> 5), i & 31)
            b = AllocatedBit.alloc(cs, None if result_value is None else bool((result_value >> i) & 1), tag)
            result_lc.append((b.variable, 1 << i))
            bits.append(Boolean.is_(b))
        cs.enforce_equal(nbits, lc, result_lc)
        return UInt32(bits[:32], None if result_value is None else result_value & 0xFFFFFFFF)
