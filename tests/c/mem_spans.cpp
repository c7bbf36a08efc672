// CPU check of ckb_zkp_amd/csrc/mem_spans.hpp against the definitions of its two predicates.  Prints "ok <sets checked>" or the
// first set on which a predicate and its definition disagree.
#include "mem_spans.hpp"

#include <cstdio>

using zkp::MemSpan;

// the definition: two spans conflict iff both are non-empty, at least one is an output and they intersect
static bool conflict(const MemSpan& a, const MemSpan& b) {
  return a.lo < a.hi && b.lo < b.hi && (a.out || b.out) && a.lo < b.hi && b.lo < a.hi;
}
static bool brute(const std::vector<MemSpan>& s) {
  for (size_t i = 0; i < s.size(); i++)
    for (size_t j = i + 1; j < s.size(); j++)
      if (conflict(s[i], s[j])) return false;
  return true;
}

static long checked = 0;
static bool check(const std::vector<MemSpan>& s) {
  checked++;
  if (zkp::outputs_disjoint(s) == brute(s)) return true;
  printf("outputs_disjoint = %d, definition = %d for", (int)zkp::outputs_disjoint(s), (int)brute(s));
  for (const MemSpan& m : s) printf(" [%lu,%lu)%s", (unsigned long)m.lo, (unsigned long)m.hi, m.out ? "out" : "in");
  printf("\n");
  return false;
}

// s, and s with up to `left` more spans: end points 0 <= lo <= hi <= 6 (lo == hi: empty), either flag, in every order of insertion
static bool exhaustive(std::vector<MemSpan>& s, int left) {
  if (!check(s)) return false;
  if (left == 0) return true;
  for (uintptr_t lo = 0; lo <= 6; lo++)
    for (uintptr_t hi = lo; hi <= 6; hi++)
      for (int out = 0; out < 2; out++) {
        s.push_back({lo, hi, out != 0});
        const bool ok = exhaustive(s, left - 1);
        s.pop_back();
        if (!ok) return false;
      }
  return true;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {                                          // xorshift64
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static bool expect(bool got, bool want, const char* what) {
  if (got != want) printf("%s: got %d, want %d\n", what, (int)got, (int)want);
  return got == want;
}

int main() {
  std::vector<MemSpan> s;
  if (!exhaustive(s, 4)) return 1;                               // 1 + 56 + 56^2 + 56^3 + 56^4 sets

  // random sets of up to 12 spans: short spans in a small range (many overlaps), long ones at large addresses (few)
  for (int it = 0; it < 6000; it++) {
    const int n = 1 + (int)(rng() % 12);
    const bool wide = it % 3 == 2;
    const uintptr_t range = wide ? (uintptr_t)1 << 40 : 64, maxlen = wide ? (uintptr_t)1 << 34 : 6;
    s.clear();
    for (int i = 0; i < n; i++) {
      const uintptr_t lo = rng() % range, len = rng() % (maxlen + 1);
      s.push_back({lo, lo + len, rng() % 4 == 0});
    }
    if (!check(s)) return 1;
  }

  bool ok = true;
  // empty spans never conflict, wherever they lie and whichever flag they carry
  ok &= expect(zkp::outputs_disjoint({{0, 8, true}, {4, 4, true}, {4, 4, false}, {6, 2, true}}), true, "empty spans inside an output");
  ok &= expect(zkp::outputs_disjoint({{0, 0, true}, {0, 0, true}}), true, "two empty outputs at one address");
  ok &= expect(zkp::outputs_disjoint({}), true, "no span");
  // equal starts, input and output in both insertion orders
  ok &= expect(zkp::outputs_disjoint({{4, 8, false}, {4, 6, true}}), false, "equal starts, input first");
  ok &= expect(zkp::outputs_disjoint({{4, 6, true}, {4, 8, false}}), false, "equal starts, output first");
  ok &= expect(zkp::outputs_disjoint({{4, 8, false}, {4, 6, false}}), true, "equal starts, two inputs");
  ok &= expect(zkp::outputs_disjoint({{4, 8, true}, {4, 8, true}}), false, "one output twice");
  // nested
  ok &= expect(zkp::outputs_disjoint({{0, 10, true}, {3, 5, false}}), false, "an input nested inside an output");
  ok &= expect(zkp::outputs_disjoint({{3, 5, true}, {0, 10, false}}), false, "an output nested inside an input");
  ok &= expect(zkp::outputs_disjoint({{0, 10, false}, {3, 5, false}, {10, 12, true}}), true, "nested inputs, an output behind them");
  // an output behind a short input that a longer, earlier input still covers
  ok &= expect(zkp::outputs_disjoint({{0, 10, false}, {2, 4, false}, {6, 8, true}}), false, "an output inside the earlier of two inputs");
  // touching
  ok &= expect(zkp::outputs_disjoint({{0, 4, true}, {4, 8, true}, {8, 12, false}}), true, "touching spans");

  // same_or_disjoint: the same start, or no common byte
  for (uintptr_t a = 0; a <= 8; a++)
    for (size_t an = 0; an <= 5; an++)
      for (uintptr_t b = 0; b <= 8; b++)
        for (size_t bn = 0; bn <= 5; bn++) {
          const bool want = a == b || a + an <= b || b + bn <= a;
          bool meet = false;                                     // some byte in both, counted one by one
          for (uintptr_t x = 0; x < 16; x++) meet |= a <= x && x < a + an && b <= x && x < b + bn;
          // with positive lengths "no common byte" is the same as "do not meet"; an empty vector is never read or written
          if (an && bn && want != (a == b || !meet)) {
            printf("same_or_disjoint's rule and the byte count disagree at %lu+%zu, %lu+%zu\n", (unsigned long)a, an, (unsigned long)b, bn);
            return 1;
          }
          if (zkp::same_or_disjoint(a, an, b, bn) != want) {
            printf("same_or_disjoint(%lu, %zu, %lu, %zu) = %d\n", (unsigned long)a, an, (unsigned long)b, bn, (int)!want);
            return 1;
          }
          checked++;
        }
  if (!ok) return 1;
  printf("ok %ld\n", checked);
  return 0;
}
