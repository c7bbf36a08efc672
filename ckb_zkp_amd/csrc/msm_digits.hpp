// K5 digit scan (msm.hip): signed c-bit window digits of one scalar, with ark's `into_repr()` fused as from_mont().  Shared by the
// level-1 sort passes of the large-MSM pipeline (msm.hip) and the batched small variable-base MSM (msm_small.hip).
#pragma once
#include "field_dev.hpp"

namespace zkp {

// Signed c-bit digits of one scalar, produced on the fly inside BOTH level-1 sort passes (histogram and scatter):
// the (bucket, point) entries are never materialised unsorted, so the scan reads 32 B per scalar (twice) and writes
// one 8-B (low key, point | sign) word per entry.  ark's `into_repr()` (prover.rs:150-161) is the fused from_mont().
struct DigitIter {
  uint32_t v[8];
  uint32_t carry;
  // window w: the first `wide` windows are c bits wide, the others c - 1 (BasesEntry::wide); nb = 2^(c-1)
  __device__ __forceinline__ void next(int w, int c, int wide, uint32_t nb, uint32_t& key, uint32_t& neg) {
    const int cw = w < wide ? c : c - 1;
    const int bit = w < wide ? w * c : wide * c + (w - wide) * (c - 1);
    const int limb = bit >> 5, sh = bit & 31;
    uint32_t d = 0;
    if (limb < 8) {
      uint64_t two = v[limb];
      if (limb + 1 < 8) two |= (uint64_t)v[limb + 1] << 32;
      d = (uint32_t)(two >> sh) & ((1u << cw) - 1);
    }
    d += carry;
    neg = 0;
    if (d > (1u << (cw - 1))) {
      d = (1u << cw) - d;
      neg = 1;
      carry = 1;
    } else {
      carry = 0;
    }
    key = d == 0 ? nb : d - 1;                      // nb == sentinel (zero digit)
  }
};
template <class FrP>
__device__ __forceinline__ DigitIter load_scalar(const uint32_t* __restrict__ scalars, size_t i, int montgomery) {
  Fp<FrP> s = Fp<FrP>::load(scalars + i * 8);
  if (montgomery) s = s.from_mont();
  DigitIter it;
#pragma unroll
  for (int l = 0; l < 8; l++) it.v[l] = s.v[l];
  it.carry = 0;
  return it;
}

}  // namespace zkp
