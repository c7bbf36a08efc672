// Sum-check rounds over dense multilinear Fr tables and eq tables (sumcheck.hip): the host entries behind
// zkp_fr_sumcheck_round_dev / zkp_fr_eq_evals_dev.  Fr only: one object serves both curves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

constexpr size_t SC_MAX_TERMS = 256;      // terms per call
constexpr int SC_MAX_LOG = 28;            // table length <= 2^28, eq table of <= 28 variables

// after the NULL checks of capi.hip: checks every other rule, then binds and / or evaluates; returns when evals_out_host is written
void fr_sumcheck_round(zkp_ctx* ctx, int curve, int kind, size_t count, uint64_t* const* tables_dev, size_t len,
                       const uint64_t* bind_host, uint64_t* evals_out_host);
// out_dev[idx] = prod_i (bit_{k-1-i}(idx) ? r[i] : 1 - r[i]), idx < 2^k
void fr_eq_evals(zkp_ctx* ctx, int curve, const uint64_t* r_host, size_t k, uint64_t* out_dev);

}  // namespace zkp
