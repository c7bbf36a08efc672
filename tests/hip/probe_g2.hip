// G2 point layer on unsaturated limbs: xyzz_madd_u2 + xyzz_u2_degenerate (unsat_dev.hpp), BkPoint<Fp2<P>> (bucket_dev.hpp) and
// quad_add_mem2 (coop_dev.hpp; 9-limb fields only, as in the product).  One object per (base field, part):
// -DPROBE_CURVE=0 (Bn254Fq) / 1 (Bls381Fq), -DPROBE_G2_PART=0 (accumulate, conversions, register forms) / 1 (memory forms).
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
using U = Fu<P>;
using F = Fp2<P>;
using Bk = BkPoint<F>;
constexpr int L = U::L, N = P::N, PT = 8 * L;
static_assert(Bk::BYTES == 4 * PT, "point layout");

#if PROBE_G2_PART == 0
// in: acc x.c0 | x.c1 | y.c0 | y.c1 | zz.c0 | zz.c1 | zzz.c0 | zzz.c1, inf, affine X.c0 | X.c1 | Y.c0 | Y.c1 (saturated), negm
// out: acc (same order), inf, return value, xyzz_u2_degenerate(acc)
struct MaddU2 {
  static constexpr int NIN = PT + 1 + 4 * N + 1, NOUT = PT + 3, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    XYZZu2<P> acc;
    acc.x = {{ld_fu<P>(in)}, {ld_fu<P>(in + L)}};
    acc.y = {{ld_fu<P>(in + 2 * L)}, {ld_fu<P>(in + 3 * L)}};
    acc.zz = {{ld_fu<P>(in + 4 * L)}, {ld_fu<P>(in + 5 * L)}};
    acc.zzz = {{ld_fu<P>(in + 6 * L)}, {ld_fu<P>(in + 7 * L)}};
    acc.inf = in[PT] != 0;
    const uint32_t* q = in + PT + 1;
    const bool ret = xyzz_madd_u2<P>(acc, U::from_sat(ld_fp<P>(q)), U::from_sat(ld_fp<P>(q + N)), U::from_sat(ld_fp<P>(q + 2 * N)),
                                     U::from_sat(ld_fp<P>(q + 3 * N)), q[4 * N]);
    st_fu<P>(out, acc.x.c0.f);
    st_fu<P>(out + L, acc.x.c1.f);
    st_fu<P>(out + 2 * L, acc.y.c0.f);
    st_fu<P>(out + 3 * L, acc.y.c1.f);
    st_fu<P>(out + 4 * L, acc.zz.c0.f);
    st_fu<P>(out + 5 * L, acc.zz.c1.f);
    st_fu<P>(out + 6 * L, acc.zzz.c0.f);
    st_fu<P>(out + 7 * L, acc.zzz.c1.f);
    out[PT] = acc.inf ? 1u : 0u;
    out[PT + 1] = ret ? 1u : 0u;
    out[PT + 2] = xyzz_u2_degenerate<P>(acc) ? 1u : 0u;
  }
};
__device__ __forceinline__ F ld_f2(const uint32_t* p) { return {ld_fp<P>(p), ld_fp<P>(p + N)}; }
__device__ __forceinline__ void st_f2(uint32_t* p, const F& a) {
  st_fp<P>(p, a.c0);
  st_fp<P>(p + N, a.c1);
}
struct BkFromSat {
  static constexpr int NIN = 8 * N, NOUT = PT, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const XYZZ<F> s{ld_f2(in), ld_f2(in + 2 * N), ld_f2(in + 4 * N), ld_f2(in + 6 * N)};
    Bk::from_sat(s).store(out);
  }
};
struct BkToSat {
  static constexpr int NIN = PT, NOUT = 8 * N + 1, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const XYZZ<F> s = Bk::load(in).to_sat();
    st_f2(out, s.x);
    st_f2(out + 2 * N, s.y);
    st_f2(out + 4 * N, s.zz);
    st_f2(out + 6 * N, s.zzz);
    out[8 * N] = s.is_inf() ? 1u : 0u;
  }
};
struct BkAdd {
  static constexpr int NIN = 2 * PT, NOUT = PT, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    Bk a = Bk::load(in);
    a.add(Bk::load(in + PT));
    a.store(out);
  }
};
struct BkDbl {
  static constexpr int NIN = PT, NOUT = PT, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) { Bk::load(in).dbl().store(out); }
};
#else
// operands in memory: the out row holds a | b | spare on entry; in[0] chooses where the result goes (0 spare, 1 over a, 2 over b)
__device__ __forceinline__ uint32_t* mem_dst(uint32_t* out, uint32_t mode) { return out + (mode == 1 ? 0 : mode == 2 ? PT : 2 * PT); }
template <bool QUAD>
struct AddMem {
  static constexpr int NIN = 1, NOUT = 3 * PT, LANES = QUAD ? 4 : 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int role) {
    const char *a = (const char*)out, *b = (const char*)(out + PT);
    char* dst = (char*)mem_dst(out, in[0]);
    if constexpr (QUAD) quad_add_mem2<P>(a, b, dst, role);
    else Bk::add_mem(a, b, dst);
  }
};
struct DblMem {
  static constexpr int NIN = 1, NOUT = 3 * PT, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    Bk::dbl_mem((const char*)out, (char*)mem_dst(out, in[0] == 1 ? 1 : 0));
  }
};
#endif

}  // namespace

int PROBE_G2_ENTRY(PROBE_ARGS) {
  if (field != FIELD) return PROBE_UNKNOWN;
#if PROBE_G2_PART == 0
  PROBE_OP("xyzz_madd_u2", MaddU2);
  PROBE_OP("bk2_from_sat", BkFromSat);
  PROBE_OP("bk2_to_sat", BkToSat);
  PROBE_OP("bk2_add", BkAdd);
  PROBE_OP("bk2_dbl", BkDbl);
#else
  PROBE_OP("bk2_add_mem", AddMem<false>);
  PROBE_OP("bk2_dbl_mem", DblMem);
#if PROBE_CURVE == 0
  PROBE_OP("quad_add_mem2", AddMem<true>);
#endif
#endif
  return PROBE_UNKNOWN;
}

}  // namespace probe
