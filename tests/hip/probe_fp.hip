// Saturated layer: Fp<P> and Fp2<P> of field_dev.hpp.  Compiled twice, with and without -DZKP_INLINE_MUL (the two forms of
// fp_mul the product's translation units use); PROBE_FP_ENTRY names the entry of this build.
#include "probe_common.hpp"

namespace probe {
namespace {

template <class P, int OP>
struct FpBin {
  static constexpr int NIN = 2 * P::N, NOUT = P::N, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const Fp<P> a = ld_fp<P>(in), b = ld_fp<P>(in + P::N);
    st_fp<P>(out, OP == 0 ? a + b : OP == 1 ? a - b : a * b);
  }
};
template <class P, int OP>
struct FpUn {
  static constexpr int NIN = P::N, NOUT = P::N, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const Fp<P> a = ld_fp<P>(in);
    Fp<P> r;
    if constexpr (OP == 0) r = a.neg();
    else if constexpr (OP == 1) r = a.dbl();
    else if constexpr (OP == 2) r = a.sqr();
    else if constexpr (OP == 3) r = Fp<P>::reduce_once(a);
    else if constexpr (OP == 4) r = a.to_mont();
    else if constexpr (OP == 5) r = a.from_mont();
    else r = a.inv();
    st_fp<P>(out, r);
  }
};
template <class P>
struct FpPow {
  static constexpr int NIN = P::N + 2, NOUT = P::N, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const uint64_t e = (uint64_t)in[P::N] | ((uint64_t)in[P::N + 1] << 32);
    st_fp<P>(out, ld_fp<P>(in).pow_u64(e));
  }
};
template <class P, int OP>
struct Fp2Op {
  static constexpr int NIN = 4 * P::N, NOUT = 2 * P::N, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const Fp2<P> a{ld_fp<P>(in), ld_fp<P>(in + P::N)}, b{ld_fp<P>(in + 2 * P::N), ld_fp<P>(in + 3 * P::N)};
    Fp2<P> r;
    if constexpr (OP == 0) r = a * b;
    else if constexpr (OP == 1) r = a.sqr();
    else r = a.inv();
    st_fp<P>(out, r.c0);
    st_fp<P>(out + P::N, r.c1);
  }
};

template <class P>
int fp_ops(PROBE_ARGS) {
  (void)field;
  PROBE_OP("fp_add", FpBin<P, 0>);
  PROBE_OP("fp_sub", FpBin<P, 1>);
  PROBE_OP("fp_mul", FpBin<P, 2>);
  PROBE_OP("fp_neg", FpUn<P, 0>);
  PROBE_OP("fp_dbl", FpUn<P, 1>);
  PROBE_OP("fp_sqr", FpUn<P, 2>);
  PROBE_OP("fp_reduce_once", FpUn<P, 3>);
  PROBE_OP("fp_to_mont", FpUn<P, 4>);
  PROBE_OP("fp_from_mont", FpUn<P, 5>);
  PROBE_OP("fp_inv", FpUn<P, 6>);
  PROBE_OP("fp_pow_u64", FpPow<P>);
  return PROBE_UNKNOWN;
}
template <class P>
int fp2_ops(PROBE_ARGS) {
  (void)field;
  PROBE_OP("fp2_mul", Fp2Op<P, 0>);
  PROBE_OP("fp2_sqr", Fp2Op<P, 1>);
  PROBE_OP("fp2_inv", Fp2Op<P, 2>);
  return PROBE_UNKNOWN;
}

}  // namespace

int PROBE_FP_ENTRY(PROBE_ARGS) {
  int st = PROBE_UNKNOWN;
  if (field == 0) st = fp_ops<Bn254Fq>(op, field, n, in, in_stride, out, out_stride);
  if (field == 1) st = fp_ops<Bn254Fr>(op, field, n, in, in_stride, out, out_stride);
  if (field == 2) st = fp_ops<Bls381Fq>(op, field, n, in, in_stride, out, out_stride);
  if (field == 3) st = fp_ops<Bls381Fr>(op, field, n, in, in_stride, out, out_stride);
  if (st != PROBE_UNKNOWN) return st;
  if (field == 0) st = fp2_ops<Bn254Fq>(op, field, n, in, in_stride, out, out_stride);
  if (field == 2) st = fp2_ops<Bls381Fq>(op, field, n, in, in_stride, out, out_stride);
  return st;
}

}  // namespace probe
