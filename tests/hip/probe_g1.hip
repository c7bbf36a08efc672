// G1 point layer on unsaturated limbs: xyzz_madd_u + xyzz_u_degenerate (unsat_dev.hpp), BkPoint<Fp<P>> (bucket_dev.hpp) and the
// quad-cooperative forms (coop_dev.hpp).  One object per base field: -DPROBE_CURVE=0 (Bn254Fq) / 1 (Bls381Fq).
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
using F = Fp<P>;
using Bk = BkPoint<F>;
constexpr int L = U::L, N = P::N, PT = 4 * L;
static_assert(Bk::BYTES == 4 * PT, "point layout");

// in: acc x | y | zz | zzz, inf, affine X | Y (saturated Montgomery words, as the window table holds them), negm
// out: acc x | y | zz | zzz, inf, return value, xyzz_u_degenerate(acc)
struct MaddU {
  static constexpr int NIN = PT + 1 + 2 * N + 1, NOUT = PT + 3, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    XYZZu<P> acc;
    acc.x = {ld_fu<P>(in)};
    acc.y = {ld_fu<P>(in + L)};
    acc.zz = {ld_fu<P>(in + 2 * L)};
    acc.zzz = {ld_fu<P>(in + 3 * L)};
    acc.inf = in[PT] != 0;
    const F ax = ld_fp<P>(in + PT + 1), ay = ld_fp<P>(in + PT + 1 + N);
    const bool ret = xyzz_madd_u<P>(acc, U::from_sat(ax), U::from_sat(ay), in[PT + 1 + 2 * N]);
    st_fu<P>(out, acc.x.f);
    st_fu<P>(out + L, acc.y.f);
    st_fu<P>(out + 2 * L, acc.zz.f);
    st_fu<P>(out + 3 * L, acc.zzz.f);
    out[PT] = acc.inf ? 1u : 0u;
    out[PT + 1] = ret ? 1u : 0u;
    out[PT + 2] = xyzz_u_degenerate<P>(acc) ? 1u : 0u;
  }
};
struct BkFromSat {
  static constexpr int NIN = 4 * N, NOUT = PT, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const XYZZ<F> s{ld_fp<P>(in), ld_fp<P>(in + N), ld_fp<P>(in + 2 * N), ld_fp<P>(in + 3 * N)};
    Bk::from_sat(s).store(out);
  }
};
struct BkToSat {
  static constexpr int NIN = PT, NOUT = 4 * N + 1, LANES = 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int) {
    const XYZZ<F> s = Bk::load(in).to_sat();
    st_fp<P>(out, s.x);
    st_fp<P>(out + N, s.y);
    st_fp<P>(out + 2 * N, s.zz);
    st_fp<P>(out + 3 * N, s.zzz);
    out[4 * N] = s.is_inf() ? 1u : 0u;
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
// operands in memory: the out row holds a | b | spare on entry; in[0] chooses where the result goes (0 spare, 1 over a, 2 over b)
__device__ __forceinline__ uint32_t* mem_dst(uint32_t* out, uint32_t mode) { return out + (mode == 1 ? 0 : mode == 2 ? PT : 2 * PT); }
template <bool QUAD>
struct AddMem {
  static constexpr int NIN = 1, NOUT = 3 * PT, LANES = QUAD ? 4 : 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int role) {
    const char *a = (const char*)out, *b = (const char*)(out + PT);
    char* dst = (char*)mem_dst(out, in[0]);
    if constexpr (QUAD) quad_add_mem<P>(a, b, dst, role);
    else Bk::add_mem(a, b, dst);
  }
};
template <bool QUAD>
struct DblMem {
  static constexpr int NIN = 1, NOUT = 3 * PT, LANES = QUAD ? 4 : 1;
  static __device__ void run(const uint32_t* in, uint32_t* out, int role) {
    char* dst = (char*)mem_dst(out, in[0] == 1 ? 1 : 0);
    if constexpr (QUAD) quad_dbl_mem<P>((const char*)out, dst, role);
    else Bk::dbl_mem((const char*)out, dst);
  }
};

}  // namespace

int PROBE_G1_ENTRY(PROBE_ARGS) {
  if (field != FIELD) return PROBE_UNKNOWN;
  PROBE_OP("xyzz_madd_u", MaddU);
  PROBE_OP("bk_from_sat", BkFromSat);
  PROBE_OP("bk_to_sat", BkToSat);
  PROBE_OP("bk_add", BkAdd);
  PROBE_OP("bk_dbl", BkDbl);
  PROBE_OP("bk_add_mem", AddMem<false>);
  PROBE_OP("bk_dbl_mem", DblMem<false>);
  PROBE_OP("quad_add_mem", AddMem<true>);
  PROBE_OP("quad_dbl_mem", DblMem<true>);
  return PROBE_UNKNOWN;
}

}  // namespace probe
