// The host-side plan of the C fold of a Groth16 key (groth16_key.hip fold_c_into_l): what every column of C costs the fold kernel, where
// the cut between the kernel's columns and the heavy ones lies, and C in column order on either side of that cut.  Pure host
// arithmetic on integers without HIP: tests/c/fold_plan.cpp includes this header alone and compares it with restatements of the
// definitions.  Field elements are 32-byte words that are only ever compared and copied, so no field type is needed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

namespace zkp {

// 1 / 2 / 0: the 32-byte coefficient is `one` / `minus_one` / anything else (the kernel's `kind` of a CSC entry)
inline uint8_t fold_coeff_kind(const uint64_t* coeff, const void* one, const void* minus_one) {
  if (memcmp(coeff, one, 32) == 0) return 1;
  if (memcmp(coeff, minus_one, 32) == 0) return 2;
  return 0;
}

// cost[m] of variable m (column m of C, nz of them) in point operations of the lane that walks it: 1 for an entry whose coefficient
// is `one` or `minus_one`, 380 for any other.  col / coeff: the nnz entries of C's CSR, 4 words per coefficient.  An entry whose
// column is no variable counts nowhere: fold_build_csc refuses such a matrix.
inline std::vector<uint64_t> fold_column_costs(size_t nz, size_t nnz, const uint32_t* col, const uint64_t* coeff, const void* one,
                                               const void* minus_one) {
  std::vector<uint64_t> cost(nz, 0);
  for (size_t e = 0; e < nnz; e++)
    if (col[e] < nz) cost[col[e]] += fold_coeff_kind(coeff + e * 4, one, minus_one) ? 1 : 380;       // 255 doublings + ~125 additions
  return cost;
}

// HEAVY columns: the kernel gives one lane per variable, and that lane walks its column serially — a 255-step
// double-and-add per general coefficient.  A dense column (the constant-one variable of packing / x * x_inv = 1 constraints, any
// variable with 1e5+ entries of C) would be a single-lane chain of 1e6-1e8 point operations.  Columns above a cost threshold leave
// the kernel's CSC and take ONE variable-base MSM each (msm_var_run over the gathered G rows), subtracted on the host afterwards.
// Threshold, MEASURED in round 6 (tests/test_gpu_fuzz.py::test_groth16_key_fold_cut_is_chosen_per_key): one cost unit = one
// point operation of a single lane ≈ 8 µs alone and ≈ 16 µs when the lanes of a wave diverge over different coefficients (40 columns
// x 57 000 units: 0.45 s; 300 x 53 200: 0.85 s), while a heavy column = host gather + H2D + msm_var_run + sync ≈ 1.7-3 ms ≈ 150 units,
// one after the other.  The fixed 50 000 of round 5 was therefore far too HIGH for the common case (a handful of dense columns: each
// up to 0.8 s of kernel chain instead of a 2 ms MSM) and only right when there are hundreds of them.  So the cut is chosen per key:
// with the column costs sorted descending, k heavy columns cost about cost[k] + 150 k — the k that minimises it, never cutting below
// 1000 (≈ 10 ms of chain).  12 columns of 38 000: twelve MSMs (≈ 30 ms) instead of a 0.3-0.6 s chain; 3000 columns of 50 000 stay in
// the kernel (≈ 0.8 s, side by side) instead of 5 s of serial MSMs.
// fixed > 0 (zkp_ctx_config.c_fold_heavy_cost / ZKP_LFOLD_HEAVY_COST) fixes the threshold instead.
// -> the threshold: a column is heavy when its cost is ABOVE it
inline uint64_t fold_heavy_cut(const std::vector<uint64_t>& costs, uint64_t fixed) {
  if (fixed > 0) return fixed;
  const uint64_t floor_cost = 1000, per_msm = 150;
  std::vector<uint64_t> big;
  for (uint64_t c : costs)
    if (c > floor_cost) big.push_back(c);
  std::sort(big.begin(), big.end(), std::greater<uint64_t>());
  uint64_t cut = floor_cost;                                 // k = all of `big` heavy
  uint64_t best = floor_cost + per_msm * big.size();
  for (size_t k = 0; k < big.size(); k++)                    // k heavy columns, the kernel's longest chain is big[k]
    if (big[k] + per_msm * k < best) {
      best = big[k] + per_msm * k;
      cut = big[k];
    }
  return cut;
}

// C in column order (column = variable, inputs ++ aux; rows ascending), split at the cut
struct FoldCsc {
  // the light columns, what the fold kernel walks: entries col_ptr[m] .. col_ptr[m + 1] of rows / kind / coeff belong to variable m.
  // kind 1 / 2: the coefficient is one / minus one; 0: the 8 Montgomery words in coeff (the kernel converts).  rows, kind and coeff
  // have room for every entry of C (at least one)
  std::vector<uint32_t> col_ptr, rows, coeff;
  std::vector<uint8_t> kind;
  // the heavy columns, ascending, and their (row, entry of the CSR) lists: 8 bytes per entry; the points and coefficients of ONE
  // column at a time are gathered right before its MSM (gathering every heavy column up front held 100 bytes per entry
  // on the host)
  std::vector<uint32_t> heavy_cols;
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> heavy;
};

// false: an entry of C names a column >= nz (the caller's ZKP_ERR_BAD_ARG); *out is then unspecified.
// costs: fold_column_costs of the same matrix; cut: fold_heavy_cut's.
inline bool fold_build_csc(size_t nz, uint32_t num_rows, const uint32_t* row_ptr, const uint32_t* col, const uint64_t* coeff,
                           const void* one, const void* minus_one, const std::vector<uint64_t>& costs, uint64_t cut, FoldCsc* out) {
  const size_t nnz = row_ptr[num_rows];
  out->col_ptr.assign(nz + 1, 0);
  out->rows.assign(std::max<size_t>(nnz, 1), 0);
  out->coeff.assign(std::max<size_t>(nnz, 1) * 8, 0);
  out->kind.assign(std::max<size_t>(nnz, 1), 0);
  out->heavy_cols.clear();
  for (size_t e = 0; e < nnz; e++)
    if (col[e] >= nz) return false;
  std::vector<uint32_t> slot(nz, UINT32_MAX);               // heavy column -> its index in heavy_cols
  for (size_t m = 0; m < nz; m++)
    if (costs[m] > cut) {
      slot[m] = (uint32_t)out->heavy_cols.size();
      out->heavy_cols.push_back((uint32_t)m);
    }
  out->heavy.assign(out->heavy_cols.size(), {});
  for (uint32_t k = 0; k < num_rows; k++)
    for (uint32_t e = row_ptr[k]; e < row_ptr[k + 1]; e++) {
      if (slot[col[e]] != UINT32_MAX) out->heavy[slot[col[e]]].emplace_back(k, e);
      else out->col_ptr[col[e] + 1]++;                       // (counts, before the prefix sum below)
    }
  for (size_t m = 0; m < nz; m++) out->col_ptr[m + 1] += out->col_ptr[m];
  std::vector<uint32_t> cur(out->col_ptr.begin(), out->col_ptr.end() - 1);
  for (uint32_t k = 0; k < num_rows; k++)
    for (uint32_t e = row_ptr[k]; e < row_ptr[k + 1]; e++) {
      if (slot[col[e]] != UINT32_MAX) continue;
      const uint32_t pos = cur[col[e]]++;
      out->rows[pos] = k;
      out->kind[pos] = fold_coeff_kind(coeff + (size_t)e * 4, one, minus_one);
      if (!out->kind[pos]) memcpy(&out->coeff[(size_t)pos * 8], coeff + (size_t)e * 4, 32);       // Montgomery words; the kernel converts
    }
  return true;
}

}  // namespace zkp
