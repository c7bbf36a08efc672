// The aliasing rules of the entry points that write through caller pointers.  Pure host code without HIP: tests/c/mem_spans.cpp
// checks both predicates on the CPU against their definitions.  fr_dev.hpp turns the first into an argument rule.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace zkp {

struct MemSpan {
  uintptr_t lo, hi;        // bytes [lo, hi); lo >= hi: empty
  bool out;                // the call writes it
};

// Outputs overlap nothing; inputs may overlap each other; empty spans never conflict.  Sorted by start, outputs first on equal
// starts, an output must begin at or after the end of everything before it and an input at or after the end of every output before it.
inline bool outputs_disjoint(std::vector<MemSpan> spans) {
  std::sort(spans.begin(), spans.end(), [](const MemSpan& a, const MemSpan& b) { return a.lo != b.lo ? a.lo < b.lo : a.out > b.out; });
  uintptr_t end_any = 0, end_out = 0;
  for (const MemSpan& sp : spans) {
    if (sp.lo >= sp.hi) continue;
    if (sp.lo < (sp.out ? end_any : end_out)) return false;
    end_any = std::max(end_any, sp.hi);
    if (sp.out) end_out = std::max(end_out, sp.hi);
  }
  return true;
}

// a call that reads index i of a before it writes index i of b: [a, a + an) and [b, b + bn) (bytes) start together or do not meet
inline bool same_or_disjoint(uintptr_t a, size_t an, uintptr_t b, size_t bn) { return a == b || a + an <= b || b + bn <= a; }

}  // namespace zkp
