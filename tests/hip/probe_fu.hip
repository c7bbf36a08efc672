// Unsaturated layer: the value operations, conversions and predicates of Fu<P> (unsat_dev.hpp), for the four fields, with the M's
// and K's the product's call sites use.  PROBE_FU_ENTRY / PROBE_FU_PART let the builder split the fields over parallel objects.
#include "probe_common.hpp"

namespace probe {
namespace {

// OP: 0 mul, 1 sqr, 2 mul_add, 3 mul_add4, 4 add, 5 dbl
template <class P, int OP, int NA>
struct FuVal {
  static constexpr int L = Fu<P>::L, NIN = NA * L, NOUT = L, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    using U = Fu<P>;
    U a[NA];
#pragma unroll
    for (int k = 0; k < NA; k++) a[k] = ld_fu<P>(in + k * L);
    U r;
    if constexpr (OP == 0) r = U::mul(a[0], a[1]);
    else if constexpr (OP == 1) r = a[0].sqr();
    else if constexpr (OP == 2) r = U::mul_add(a[0], a[1], a[2], a[3]);
    else if constexpr (OP == 3) r = U::mul_add4(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
    else if constexpr (OP == 4) r = U::add(a[0], a[1]);
    else r = a[0].dbl();
    st_fu<P>(out, r);
  }
};
// OP: 0 sub<M>, 1 sub_sub2<M>, 2 sub_sel<M> (+ one word m), 3 csub<M>, 4 sub_lazy<M>, 5 neg_lazy<M>
template <class P, int OP, int M>
struct FuSub {
  static constexpr int L = Fu<P>::L, NA = OP == 1 ? 3 : (OP == 3 || OP == 5) ? 1 : 2;
  static constexpr int NIN = NA * L + (OP == 2 ? 1 : 0), NOUT = L, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    using U = Fu<P>;
    const U a = ld_fu<P>(in);
    U r;
    if constexpr (OP == 0) r = U::template sub<M>(a, ld_fu<P>(in + L));
    else if constexpr (OP == 1) r = U::template sub_sub2<M>(a, ld_fu<P>(in + L), ld_fu<P>(in + 2 * L));
    else if constexpr (OP == 2) r = U::template sub_sel<M>(a, ld_fu<P>(in + L), in[2 * L]);
    else if constexpr (OP == 3) r = U::template csub<M>(a);
    else if constexpr (OP == 4) r = U::template sub_lazy<M>(a, ld_fu<P>(in + L));
    else r = U::template neg_lazy<M>(a);
    st_fu<P>(out, r);
  }
};
// OP: 0 from_words(a, 0), 1 from_sat, 2 from_sat_reduced
template <class P, int OP>
struct FuFrom {
  static constexpr int NIN = P::N, NOUT = Fu<P>::L, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    using U = Fu<P>;
    const Fp<P> a = ld_fp<P>(in);
    st_fu<P>(out, OP == 0 ? U::from_words(a.v, 0) : OP == 1 ? U::from_sat(a) : U::from_sat_reduced(a));
  }
};
// OP: 0 to_words, 1 to_sat
template <class P, int OP>
struct FuTo {
  static constexpr int NIN = Fu<P>::L, NOUT = P::N, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const Fu<P> a = ld_fu<P>(in);
    Fp<P> r;
    if constexpr (OP == 0) a.to_words(r.v);
    else r = a.to_sat();
    st_fp<P>(out, r);
  }
};
template <class P>
struct FuOne {
  static constexpr int NIN = 0, NOUT = Fu<P>::L, LANES = 1;
  static __device__ void run(const uint32_t*, uint32_t* out, int) { st_fu<P>(out, Fu<P>::one()); }
};
// OP: 0 is_zero_mod_p<K>, 1 is_multiple_of_p<K>, 2 maybe_multiple_of_p<K>
template <class P, int OP, int K>
struct FuPred {
  static constexpr int NIN = Fu<P>::L, NOUT = 1, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const Fu<P> a = ld_fu<P>(in);
    bool r;
    if constexpr (OP == 0) r = a.template is_zero_mod_p<K>();
    else if constexpr (OP == 1) r = a.template is_multiple_of_p<K>();
    else r = a.template maybe_multiple_of_p<K>();
    out[0] = r ? 1u : 0u;
  }
};
// ntt_mul of ntt.hip lives in a translation unit, not in a header: its body is restated here, word for word
//   Fu r = Fu::mul(Fu::from_words(x.v, 0), t); r.to_words(o.v); return Fp::reduce_once(o);
template <class P>
struct NttMul {
  static constexpr int NIN = P::N + Fu<P>::L, NOUT = P::N, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const Fp<P> x = ld_fp<P>(in);
    const Fu<P> t = ld_fu<P>(in + P::N);
    Fu<P> r = Fu<P>::mul(Fu<P>::from_words(x.v, 0), t);
    Fp<P> o;
    r.to_words(o.v);
    st_fp<P>(out, Fp<P>::reduce_once(o));
  }
};

template <class P>
int fu_ops(PROBE_ARGS) {
  (void)field;
  PROBE_OP("fu_mul", FuVal<P, 0, 2>);
  PROBE_OP("fu_sqr", FuVal<P, 1, 1>);
  PROBE_OP("fu_mul_add", FuVal<P, 2, 4>);
  PROBE_OP("fu_mul_add4", FuVal<P, 3, 8>);
  PROBE_OP("fu_add", FuVal<P, 4, 2>);
  PROBE_OP("fu_dbl", FuVal<P, 5, 1>);
  PROBE_OP("fu_sub<2>", FuSub<P, 0, 2>);
  PROBE_OP("fu_sub<4>", FuSub<P, 0, 4>);
  PROBE_OP("fu_sub<6>", FuSub<P, 0, 6>);
  PROBE_OP("fu_sub<8>", FuSub<P, 0, 8>);
  PROBE_OP("fu_sub_sub2<6>", FuSub<P, 1, 6>);
  PROBE_OP("fu_sub_sel<2>", FuSub<P, 2, 2>);
  PROBE_OP("fu_sub_sel<4>", FuSub<P, 2, 4>);
  PROBE_OP("fu_sub_sel<6>", FuSub<P, 2, 6>);
  PROBE_OP("fu_csub<2>", FuSub<P, 3, 2>);
  PROBE_OP("fu_csub<4>", FuSub<P, 3, 4>);
  PROBE_OP("fu_sub_lazy<7>", FuSub<P, 4, 7>);
  PROBE_OP("fu_sub_lazy<9>", FuSub<P, 4, 9>);
  PROBE_OP("fu_neg_lazy<3>", FuSub<P, 5, 3>);
  PROBE_OP("fu_neg_lazy<5>", FuSub<P, 5, 5>);
  PROBE_OP("fu_neg_lazy<7>", FuSub<P, 5, 7>);
  PROBE_OP("fu_from_words", FuFrom<P, 0>);
  PROBE_OP("fu_from_sat", FuFrom<P, 1>);
  PROBE_OP("fu_from_sat_reduced", FuFrom<P, 2>);
  PROBE_OP("fu_to_words", FuTo<P, 0>);
  PROBE_OP("fu_to_sat", FuTo<P, 1>);
  PROBE_OP("fu_one", FuOne<P>);
  PROBE_OP("fu_is_zero_mod_p<2>", FuPred<P, 0, 2>);
  PROBE_OP("fu_is_multiple_of_p<4>", FuPred<P, 1, 4>);
  PROBE_OP("fu_maybe_multiple_of_p<4>", FuPred<P, 2, 4>);
  PROBE_OP("fu_ntt_mul", NttMul<P>);
  return PROBE_UNKNOWN;
}

}  // namespace

int PROBE_FU_ENTRY(PROBE_ARGS) {
#if PROBE_FU_PART == 0
  if (field == 0) return fu_ops<Bn254Fq>(op, field, n, in, in_stride, out, out_stride);
  if (field == 1) return fu_ops<Bn254Fr>(op, field, n, in, in_stride, out, out_stride);
  if (field == 3) return fu_ops<Bls381Fr>(op, field, n, in, in_stride, out, out_stride);
#else
  if (field == 2) return fu_ops<Bls381Fq>(op, field, n, in, in_stride, out, out_stride);
#endif
  return PROBE_UNKNOWN;
}

}  // namespace probe
