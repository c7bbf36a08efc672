// Resident Pedersen key, row commitments and the Fr vector-matrix product (pedersen.hip): the plan of the bucket pass and the
// per-curve launch table.  Kept apart from MsmSmallVtbl / IpaVtbl so that the MSM and IPA units are not touched by it.
// No HIP type appears here: tests/c/pedersen_plan.cpp includes this header alone and prints the plan on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct zkp_ctx;
struct zkp_pedersen_key;

namespace zkp {

constexpr int PED_LANES = 64;                    // one wave per workgroup: the LDS buckets have a single writer (as msm_small)
constexpr int PED_SLOTS = 2 * PED_LANES;         // boundary slots of the segmented tree
constexpr uint32_t PED_MAX_ENTRIES = 4096;       // (generator, window) pairs of one slice: 12 bits of a sorted entry
constexpr uint32_t PED_MAX_GENS = 65536;         // == ZKP_PEDERSEN_MAX_GENS == ZKP_MSM_SMALL_MAX_G1
constexpr uint64_t PED_MAX_CELLS = (uint64_t)1 << 28;     // rows * cols of one call (commit_rows and vecmat)
constexpr uint32_t PED_LDS_MAX = 160 * 1024;     // == SMALL_LDS_MAX: the LDS of one CDNA4 compute unit
constexpr int PED_LAUNCHES = 3;                  // bucket pass, row pass, affine pass: whatever rows and cols are
constexpr uint32_t VECMAT_THREADS = 64;          // consecutive columns of one workgroup
constexpr uint32_t VECMAT_ROW_CHUNK = 32;        // rows of one workgroup (== ZKP_FR_VECMAT_ROW_CHUNK)

// Window bits per curve.  c = 8 on both: 2^(c-1) = 128 buckets are two per lane, so the bucket fold (2 additions per bucket in
// one lane, then two 6-level trees) stays a quarter of the <= 64 chunk additions a lane makes for a full slice, and the buckets,
// boundary slots and staging points (320 BkPoints: 45 / 70 KiB) leave room for two (BN254) / one (BLS12-381) workgroup per CU.
// c = 9 would put 141 instead of 124 generators into a slice (+14 %) for twice the fold and 18 / 28 KiB more LDS.
constexpr int pedersen_c(int /*curve*/) { return 8; }
// bytes of one BkPoint (bucket_dev.hpp): 4 elements of 9 x 29-bit (BN254) / 14 x 28-bit (BLS12-381) limbs
constexpr uint32_t pedersen_bk_bytes(int curve) { return curve == 0 ? 4 * 4 * 9 : 4 * 4 * 14; }

struct PedersenPlan {
  uint32_t c;          // window bits: digits in [-2^(c-1), 2^(c-1)]
  uint32_t W;          // windows: floor((256 + c) / c) as in msm_small, so W c > 256 and the top window absorbs the last carry
  uint32_t nb;         // 2^(c-1) buckets of one workgroup
  uint32_t G;          // generators of one slice at most: floor(PED_MAX_ENTRIES / W)
  uint32_t S;          // slices of one row of `cols` generators: ceil(cols / G)
  uint32_t g;          // generators of every slice but the last: ceil(cols / S) <= G (slices of one row are balanced)
  uint32_t lds_bytes;  // of one workgroup of the bucket pass (sized for G generators whatever cols is)
};

// slice j of a row covers generators [j g, min(cols, (j + 1) g)) in all W windows: every (generator, window) pair exactly once
inline PedersenPlan pedersen_plan(int curve, uint32_t cols) {
  PedersenPlan p;
  p.c = (uint32_t)pedersen_c(curve);
  p.W = (256 + p.c) / p.c;
  p.nb = 1u << (p.c - 1);
  p.G = PED_MAX_ENTRIES / p.W;
  p.S = (cols + p.G - 1) / p.G;
  p.g = p.S ? (cols + p.S - 1) / p.S : 0;
  const uint32_t E = p.G * p.W;
  // nb buckets, 2 boundary slots and one staging point per lane, the slots' keys, the histogram (nb + 1 keys, padded), the sorted
  // entries (u32) and the digit of each entry (u16)
  p.lds_bytes = (p.nb + PED_SLOTS + PED_LANES) * pedersen_bk_bytes(curve) + 4 * PED_SLOTS + 4 * (p.nb + 4) + 4 * E + 2 * E;
  return p;
}

struct PedersenVtbl {
  // after the NULL checks of capi.hip: every other rule, then the work
  void (*key_create)(zkp_ctx* ctx, const uint64_t* gens_xy_host, const uint8_t* gens_inf_host, size_t n_gens,
                     const uint64_t* h_xy_host, zkp_pedersen_key** out);                        // returns when the tables are built
  void (*commit_rows)(zkp_ctx* ctx, const zkp_pedersen_key* key, const uint64_t* scalars_dev, size_t rows, size_t cols,
                      const uint64_t* blinds_dev, uint64_t* out_xy_dev, uint8_t* out_inf_dev);    // launches only
  void (*vecmat)(zkp_ctx* ctx, const uint64_t* l_dev, const uint64_t* m_dev, size_t rows, size_t cols, uint64_t* out_dev);   // launches only
};

const PedersenVtbl* pedersen_vtbl_c0();          // pedersen.hip, -DZKP_CFG_CURVE=0
const PedersenVtbl* pedersen_vtbl_c1();          // pedersen.hip, -DZKP_CFG_CURVE=1
const PedersenVtbl* pedersen_vtbl(int curve);    // throws StatusError on an unknown curve
void pedersen_key_free(zkp_ctx* ctx, zkp_pedersen_key* key);
void pedersen_key_info(const zkp_pedersen_key* key, uint64_t info[8]);
int pedersen_key_curve(const zkp_pedersen_key* key);

}  // namespace zkp
