// Saturated point arithmetic (ec_dev.hpp): XYZZ<F> over F = Fp<P> (G1) and F = Fp2<P> (G2), one method per operation, raw
// canonical Montgomery words in and out.  One object per (base field, group, part): -DPROBE_CURVE=0 (Bn254Fq) / 1 (Bls381Fq),
// -DPROBE_GROUP=1 / 2, -DPROBE_EC_PART=0 (doublings) / 1 (mixed additions) / 2 (full addition) / 3 (conversions): the inlined Fq2
// formulas compile slowly.  ZKP_INLINE_MUL as the product's msm_group unit of the same (curve, group) has it.
// A point is x | y | zz | zzz, an affine point x | y, a Jacobian point X | Y | Z; an Fp2 coordinate is c0 | c1.
#include "probe_common.hpp"

namespace probe {
namespace {

#if PROBE_CURVE == 0
using P = Bn254Fq;
constexpr int FIELD = 0;
#else
using P = Bls381Fq;
constexpr int FIELD = 2;
#endif
#if PROBE_GROUP == 1
using F = Fp<P>;
__device__ __forceinline__ F ld_f(const uint32_t* p) { return ld_fp<P>(p); }
__device__ __forceinline__ void st_f(uint32_t* p, const F& a) { st_fp<P>(p, a); }
#else
using F = Fp2<P>;
__device__ __forceinline__ F ld_f(const uint32_t* p) { return {ld_fp<P>(p), ld_fp<P>(p + P::N)}; }
__device__ __forceinline__ void st_f(uint32_t* p, const F& a) {
  st_fp<P>(p, a.c0);
  st_fp<P>(p + P::N, a.c1);
}
#endif
using Pt = XYZZ<F>;
constexpr int W = F::N;                                      // words of a coordinate
static_assert(Pt::BYTES == 16 * W && Affine<F>::BYTES == 8 * W, "point layout");

__device__ __forceinline__ Pt ld_pt(const uint32_t* p) { return {ld_f(p), ld_f(p + W), ld_f(p + 2 * W), ld_f(p + 3 * W)}; }
__device__ __forceinline__ void st_pt(uint32_t* p, const Pt& a) {
  st_f(p, a.x);
  st_f(p + W, a.y);
  st_f(p + 2 * W, a.zz);
  st_f(p + 3 * W, a.zzz);
}
__device__ __forceinline__ Affine<F> ld_aff(const uint32_t* p) { return {ld_f(p), ld_f(p + W)}; }

#if PROBE_EC_PART == 0
struct DblAffine {
  static constexpr int NIN = 2 * W, NOUT = 4 * W, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) { st_pt(out, Pt::dbl_affine(ld_aff(in))); }
};
struct Dbl {
  static constexpr int NIN = 4 * W, NOUT = 4 * W, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) { st_pt(out, ld_pt(in).dbl()); }
};
#elif PROBE_EC_PART == 1
// in: acc, affine addend
struct Madd {
  static constexpr int NIN = 6 * W, NOUT = 4 * W, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    Pt a = ld_pt(in);
    a.madd(ld_aff(in + 4 * W));
    st_pt(out, a);
  }
};
// out: acc afterwards, return value
struct MaddFast {
  static constexpr int NIN = 6 * W, NOUT = 4 * W + 1, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    Pt a = ld_pt(in);
    const bool ret = a.madd_fast(ld_aff(in + 4 * W));
    st_pt(out, a);
    out[4 * W] = ret ? 1u : 0u;
  }
};
#elif PROBE_EC_PART == 2
struct Add {
  static constexpr int NIN = 8 * W, NOUT = 4 * W, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    Pt a = ld_pt(in);
    a.add(ld_pt(in + 4 * W));
    st_pt(out, a);
  }
};
#else
struct ToAffine {
  static constexpr int NIN = 4 * W, NOUT = 2 * W, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const Affine<F> a = ld_pt(in).to_affine();
    st_f(out, a.x);
    st_f(out + W, a.y);
  }
};
// store_jacobian writes through 16-byte vector stores: it gets an aligned buffer of its own, so any out_stride will do
struct StoreJacobian {
  static constexpr int NIN = 4 * W, NOUT = 3 * W, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    __attribute__((aligned(16))) uint32_t tmp[3 * W];
    ld_pt(in).store_jacobian(tmp);
#pragma unroll
    for (int i = 0; i < 3 * W; i++) out[i] = tmp[i];
  }
};
// jac_to_xyzz is local to msm_group.hip (fold_kernel, into_affine_kernel, from_jacobian_kernel); these are its lines, copied:
//   F X = F::load(p), Y = F::load(p + F::N), Z = F::load(p + 2 * F::N);
//   if (Z.is_zero()) return XYZZ<F>::inf();
//   F zz = Z.sqr();
//   return {X, Y, zz, zz * Z};
struct FromJacobian {
  static constexpr int NIN = 3 * W, NOUT = 4 * W, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    F X = ld_f(in), Y = ld_f(in + W), Z = ld_f(in + 2 * W);
    if (Z.is_zero()) {
      st_pt(out, Pt::inf());
      return;
    }
    F zz = Z.sqr();
    st_pt(out, Pt{X, Y, zz, zz * Z});
  }
};
#endif

}  // namespace

// the operation's name carries the group: "ec_add" (G1) / "ec2_add" (G2)
#if PROBE_GROUP == 1
#define EC_NAME(x) "ec_" x
#else
#define EC_NAME(x) "ec2_" x
#endif

int PROBE_EC_ENTRY(PROBE_ARGS) {
  if (field != FIELD) return PROBE_UNKNOWN;
#if PROBE_EC_PART == 0
  PROBE_OP(EC_NAME("dbl_affine"), DblAffine);
  PROBE_OP(EC_NAME("dbl"), Dbl);
#elif PROBE_EC_PART == 1
  PROBE_OP(EC_NAME("madd"), Madd);
  PROBE_OP(EC_NAME("madd_fast"), MaddFast);
#elif PROBE_EC_PART == 2
  PROBE_OP(EC_NAME("add"), Add);
#else
  PROBE_OP(EC_NAME("to_affine"), ToAffine);
  PROBE_OP(EC_NAME("store_jacobian"), StoreJacobian);
  PROBE_OP(EC_NAME("from_jacobian"), FromJacobian);
#endif
  return PROBE_UNKNOWN;
}

}  // namespace probe
