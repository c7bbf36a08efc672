// Batched small variable-base MSM (msm_small.hip): descriptor layout and the per-(curve, group) launch table.  Kept apart from
// MsmVtbl so that the large-MSM units are not touched by it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace zkp {

constexpr int SMALL_LANES = 64;           // one wave per workgroup: the LDS buckets have a single writer
constexpr int SMALL_SLOTS = 2 * SMALL_LANES;
constexpr uint32_t SMALL_LDS_MAX = 160 * 1024;

// one entry of a batch, built on the host and uploaded once per call
struct SmallDesc {
  const uint32_t* xy;          // n affine Montgomery points (device)
  const uint8_t* inf;          // n identity flags, or nullptr
  const uint32_t* scalars;     // n x 8 words (device)
  uint32_t n;
  uint32_t c;                  // window bits; nb = 2^(c-1) buckets, digits in [-nb, nb]
  uint32_t W;                  // windows (W * c > 256: the top window absorbs the last carry)
  uint32_t S;                  // slices of `slice` points
  uint32_t first_wg;           // workgroup of (w = 0, j = 0); workgroup first_wg + w * S + j writes partial slot first_wg + w * S + j
  uint32_t pad;
};

// LDS bytes of one workgroup: nb buckets, 2 boundary slots per lane, one staging point per lane, the slots' keys, the histogram /
// cursors (nb + 1 keys incl. the zero-digit sentinel), the sorted entries (u32) and the digit of each slice entry (u16)
inline uint32_t small_lds_bytes(size_t bk_bytes, int c, uint32_t slice) {
  const uint32_t nb = 1u << (c - 1);
  return (uint32_t)((nb + SMALL_SLOTS + SMALL_LANES) * bk_bytes) + 4 * SMALL_SLOTS + 4 * (nb + 4) + 4 * slice + 2 * slice;
}

struct MsmSmallVtbl {
  size_t bk_bytes;             // BkPoint<F>::BYTES
  int jac_words;               // 32-bit words of one Jacobian result (3 fN)
  // launch 1: one workgroup per (entry, window, slice) -> partial[wg]; launch 2: one workgroup per entry -> out_jac[k]
  void (*run)(hipStream_t, const SmallDesc* desc, uint32_t count, uint32_t total_wg, uint32_t slice, int montgomery,
              uint32_t lds_bytes, char* partial, uint32_t* out_jac);
};

const MsmSmallVtbl* msm_small_vtbl(int curve, int group);     // msm.hip; throws StatusError on unknown config

}  // namespace zkp
