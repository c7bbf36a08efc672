// The polynomial work between the PLONK rounds and a proof (fr_open.hip): many polynomials evaluated at one shared point and a
// linear combination of many Fr vectors, each in one pass.  The host entries behind zkp_fr_poly_eval_many_dev /
// zkp_fr_lincomb_dev.  Fr only: one object serves both curves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

// Both entries take at most FR_OPEN_MAX_POLYS vectors of at most 2^FR_OPEN_MAX_LOG elements: the pointer / length table and the
// scalars travel as kernel arguments.
constexpr uint32_t FR_OPEN_MAX_POLYS = 32;
constexpr uint32_t FR_OPEN_MAX_LOG = 30;
// The evaluation's grid is capped like the PLONK quotient's: thread j owns the coefficients j, j + T, j + 2T, ... with
// T = THREADS * min(ceil(max ns / THREADS), MAX_BLOCKS).
constexpr uint32_t FR_OPEN_EVAL_THREADS = 256;
constexpr uint32_t FR_OPEN_EVAL_MAX_BLOCKS = 512;
// Polynomials that share one walk of the powers of z: their accumulators stay in registers (no scratch, no spills).
constexpr uint32_t FR_OPEN_EVAL_GROUP = 4;
static_assert(FR_OPEN_MAX_POLYS % FR_OPEN_EVAL_GROUP == 0, "whole groups");
constexpr uint32_t FR_OPEN_LINCOMB_THREADS = 256;

// after the NULL checks of capi.hip: every other rule, then the work
void fr_poly_eval_many(zkp_ctx* ctx, int curve, size_t count, const uint64_t* const* p_dev, const size_t* ns, const uint64_t* z_host,
                       uint64_t* out_host);                       // returns when out_host is written
void fr_lincomb(zkp_ctx* ctx, int curve, size_t count, const uint64_t* const* p_dev, const size_t* ns, const uint64_t* coeffs_host,
                uint64_t* out_dev, size_t n_out);                 // launches only, like fr_vec_op

}  // namespace zkp
