// SPARK memory-checking hashes and product circuits (spark.hip): the host entries behind zkp_fr_product_circuit_dev /
// zkp_fr_memcheck_circuits_dev.  Fr only: one object serves both curves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctx.hpp"

namespace zkp {

constexpr size_t SP_MAX_CIRCUITS = 256;   // circuits per call
constexpr int SP_MAX_LOG = 28;            // leaves per circuit <= 2^28
constexpr int SP_TAIL_LOG = 9;            // a layer of <= 2^9 elements is finished by one workgroup per circuit (the tail launch)

// element at which layer l of a circuit of n leaves starts (n >> l elements; 2n - 2 in all)
inline constexpr size_t sp_layer_offset(size_t n, int l) { return 2 * n - ((2 * n) >> l); }
// launches of one call: strided passes of up to three layers each down to 2^SP_TAIL_LOG elements, then the tail
inline constexpr int sp_launches(int log_n) { return log_n > SP_TAIL_LOG ? (log_n - SP_TAIL_LOG + 2) / 3 + 1 : 1; }

// after the NULL checks of capi.hip: checks every other rule, then builds the circuits; returns when roots_host is written.
// val_dev == NULL: layer 0 is in place (zkp_fr_product_circuit_dev) and addr_dev / ts_dev / ts_add / the gammas are not read.
void fr_spark_circuits(zkp_ctx* ctx, int curve, size_t count, const uint32_t* const* addr_dev, const uint64_t* const* val_dev,
                       const uint32_t* const* ts_dev, const uint32_t* ts_add, uint64_t* const* circuits_dev, size_t n,
                       const uint64_t* gamma1_host, const uint64_t* gamma2_host, uint64_t* roots_host);

}  // namespace zkp
