// IPA generator fold (zkp_g1_ipa_fold_dev): out[i] = (a L[i] + b R[i]).into_affine() with one pair of Fr scalars for every i — the
// `g_new` step of bullet_inner_product_proof (spartan/src/inner_product.rs:71-74, hyrax/src/commitment.rs:550-552).  Compiled once
// per curve, G1 only: -DZKP_CFG_CURVE={0,1}.
//
// Scalars, on the host once per call: a and b are GLV-decomposed (glv.hpp) into four signed magnitudes < 2^129, so that
// a L + b R = k1 L + k2 phi(L) + k3 R + k4 phi(R), and each pair (k1, k2), (k3, k4) is recoded in joint sparse form (Solinas):
// digits in {-1, 0, 1}, on average half of the positions of a pair non-zero.  The plan (<= 130 positions, one byte each, IpaPlan) is
// a kernel argument.  a and b are the same for every lane, so the digits are uniform over the wave: no divergent scalar control flow.
//
// Per pair and lane, with phi(P) = lambda P and 1 + lambda + lambda^2 = 0 (mod r), every joint digit but one is an affine point:
//   +-P = (x, +-y)    +-phi(P) = (beta x, +-y)    +-(P + phi(P)) = -+phi^2(P) = (beta^2 x, -+y)    +-(P - phi(P)): one XYZZ point
// so a lane keeps x, beta x, beta^2 x, y and P - phi(P) of both of its inputs in LDS (the only table entry that costs an addition)
// and runs ~130 doublings + ~130 additions (two pairs x 1/2 per position) on the unsaturated formulas of bucket_dev.hpp with the
// accumulator in registers.
//
// Affine output: Montgomery's trick per workgroup (one wave) over d = ZZ ZZZ, as a product tree in LDS (one product per point up,
// two down), one Fermat inversion per workgroup, then 1/ZZ = ZZZ / d and 1/ZZZ = ZZ / d.  Identities (ZZ == 0, flagged or (0, 0)
// inputs, a = 0 and b = 0) stay out of the tree and are written as zkp_fixed_base_mul_g1 writes them: words (0, 0), flag 1.
// Every output is the canonical affine form, so the result is bit-exact whatever the order of the additions.
#include <cstring>

#include "bucket_dev.hpp"
#include "ec_dev.hpp"
#include "glv.hpp"
#include "host_field.hpp"
#include "ipa.hpp"

#ifndef ZKP_CFG_CURVE
#error "compile with -DZKP_CFG_CURVE=0|1"
#endif

namespace zkp {

#if ZKP_CFG_CURVE == 0
using IpFq = Bn254Fq;
constexpr int IP_CURVE = ZKP_BN254;
#else
using IpFq = Bls381Fq;
constexpr int IP_CURVE = ZKP_BLS12_381;
#endif
using IpF = Fp<IpFq>;

#define ZKP_IP_CAT(a, b) a##b
#define ZKP_IP_SYM(name, cu) ZKP_IP_CAT(name, cu)
// the same source is compiled twice: one namespace per curve
namespace ZKP_IP_SYM(ipa_c, ZKP_CFG_CURVE) {

// LDS of one lane: per input (L, then R) x, beta x, beta^2 x, y (saturated) and P - phi(P) (BkPoint)
template <class F>
struct IpaLds {
  static constexpr int FB = 4 * F::N;
  static constexpr int SIDE = 4 * FB + BkPoint<F>::BYTES;
  static constexpr int STRIDE = 2 * SIDE + 16;   // +16 B: the 16-B reads of consecutive lanes start on different banks
};

// Digit codes of one pair (P, phi P): 0 none, 1 / 2 +-P, 3 / 4 +-phi(P), 5 / 6 +-(P + phi(P)), 7 / 8 +-(P - phi(P))
template <class F>
__device__ __forceinline__ void ipa_apply(BkPoint<F>& acc, uint32_t code, const char* side, bool skip) {
  using B = BkPoint<F>;
  using T = IpaLds<F>;
  if (code == 0 || skip) return;
  B op;
  if (code <= 6) {
    const F x = F::load(side + ((code - 1) >> 1) * T::FB);
    F y = F::load(side + 3 * T::FB);
    if (code == 2 || code == 4 || code == 5) y = y.neg();
    op = B::from_sat(XYZZ<F>::from_affine(Affine<F>{x, y}));
  } else {
    op = B::load(side + 4 * T::FB);
    if (code == 8 && !op.v.inf) op.v.y = ub_neg<4>(op.v.y);
  }
  acc.add(op);
}

// out may equal l or r (in place): a lane reads only index i of every input before it writes index i of the outputs, so no pointer
// here is __restrict__.
template <class F>
__global__ __launch_bounds__(IPA_LANES) void ipa_fold_kernel(const uint32_t* l_xy, const uint8_t* l_inf, const uint32_t* r_xy,
                                                             const uint8_t* r_inf, uint32_t n, IpaPlan plan, uint32_t* out_xy,
                                                             uint8_t* out_inf) {
  using B = BkPoint<F>;
  using T = IpaLds<F>;
  using G = GlvConst<IpFq>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * IPA_LANES + t;
  const bool act = i < n;
  char* mine = smem + (size_t)t * T::STRIDE;
  F beta;
#pragma unroll
  for (int k = 0; k < F::N; k++) beta.v[k] = G::BETA_MONT[k];
  const F beta2 = beta.sqr();

  bool skip[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const uint32_t* xy = s ? r_xy : l_xy;
    const uint8_t* inf = s ? r_inf : l_inf;
    char* sd = mine + s * T::SIDE;
    const Affine<F> p = act ? Affine<F>::load(xy + i * (2 * F::N)) : Affine<F>::inf();
    skip[s] = !act || (inf && inf[i]) || p.is_inf();
    if (!skip[s]) {
      const F bx = beta * p.x;
      p.x.store(sd);
      bx.store(sd + T::FB);
      (beta2 * p.x).store(sd + 2 * T::FB);
      p.y.store(sd + 3 * T::FB);
      B d = B::from_sat(XYZZ<F>::from_affine(p));                                  // P - phi(P)
      d.add(B::from_sat(XYZZ<F>::from_affine(Affine<F>{bx, p.y.neg()})));
      d.store(sd + 4 * T::FB);
    }
  }

  B acc = B::inf();
  for (int j = (int)plan.ndig - 1; j >= 0; j--) {
    acc = acc.dbl();
    const uint32_t code = plan.dig[j];
    ipa_apply<F>(acc, code & 15u, mine, skip[0]);
    ipa_apply<F>(acc, code >> 4, mine + T::SIDE, skip[1]);
  }

  // batch inversion of d = ZZ ZZZ over the workgroup: node k of the tree at tree + k FB, leaves [IPA_LANES, 2 IPA_LANES)
  const XYZZ<F> p = acc.to_sat();
  const bool id = !act || p.is_inf();
  __syncthreads();                                               // the tables are dead
  char* tree = smem;
  (id ? F::one() : p.zz * p.zzz).store(tree + (size_t)(IPA_LANES + t) * T::FB);
  __syncthreads();
  for (int h = IPA_LANES / 2; h >= 1; h >>= 1) {
    if (t < h) {
      const int k = h + t;
      (F::load(tree + (size_t)(2 * k) * T::FB) * F::load(tree + (size_t)(2 * k + 1) * T::FB)).store(tree + (size_t)k * T::FB);
    }
    __syncthreads();
  }
  if (t == 0) F::load(tree + T::FB).inv().store(tree + T::FB);
  __syncthreads();
  for (int h = 1; h < IPA_LANES; h <<= 1) {                      // node k holds 1 / (its product): its children get theirs
    if (t < h) {
      const int k = h + t;
      const F ik = F::load(tree + (size_t)k * T::FB);
      const F a = F::load(tree + (size_t)(2 * k) * T::FB), b = F::load(tree + (size_t)(2 * k + 1) * T::FB);
      (ik * b).store(tree + (size_t)(2 * k) * T::FB);
      (ik * a).store(tree + (size_t)(2 * k + 1) * T::FB);
    }
    __syncthreads();
  }
  if (!act) return;
  uint32_t* o = out_xy + i * (2 * F::N);
  if (id) {
    Affine<F>::inf().store(o);
    out_inf[i] = 1;
    return;
  }
  const F e = F::load(tree + (size_t)(IPA_LANES + t) * T::FB);   // 1 / (ZZ ZZZ)
  Affine<F>{p.x * (e * p.zzz), p.y * (e * p.zz)}.store(o);
  out_inf[i] = 0;
}

// ------------------------------------------------------------------------------------------- host: plan
// Joint sparse form of (k0, k1) (Solinas 2001; Hankerson-Menezes-Vanstone Alg. 3.50): k_s = sum_j u_s[j] 2^j, u in {-1, 0, 1}.
int jsf(const uint32_t* k0_in, const uint32_t* k1_in, int8_t* u0, int8_t* u1) {
  uint32_t k[2][5];
  memcpy(k[0], k0_in, sizeof k[0]);
  memcpy(k[1], k1_in, sizeof k[1]);
  int d[2] = {0, 0}, len = 0;
  auto live = [&](int s) {
    uint32_t o = (uint32_t)d[s];
    for (int w = 0; w < 5; w++) o |= k[s][w];
    return o != 0;
  };
  while (live(0) || live(1)) {
    ZKP_REQUIRE(len < IPA_MAX_DIG, ZKP_ERR_DEVICE);             // cannot happen for |k| < 2^129
    const int l0 = (int)((k[0][0] & 7u) + d[0]) & 7, l1 = (int)((k[1][0] & 7u) + d[1]) & 7;   // (k + d) mod 8
    int v0 = 0, v1 = 0;
    if (l0 & 1) {
      v0 = (l0 & 3) == 1 ? 1 : -1;
      if ((l0 == 3 || l0 == 5) && (l1 & 3) == 2) v0 = -v0;
    }
    if (l1 & 1) {
      v1 = (l1 & 3) == 1 ? 1 : -1;
      if ((l1 == 3 || l1 == 5) && (l0 & 3) == 2) v1 = -v1;
    }
    if (2 * d[0] == 1 + v0) d[0] = 1 - d[0];
    if (2 * d[1] == 1 + v1) d[1] = 1 - d[1];
    for (int s = 0; s < 2; s++)
      for (int w = 0; w < 5; w++) k[s][w] = (k[s][w] >> 1) | (w < 4 ? k[s][w + 1] << 31 : 0u);
    u0[len] = (int8_t)v0;
    u1[len] = (int8_t)v1;
    len++;
  }
  return len;
}

// code of the joint digit (e0 P + e1 phi(P)), signs applied (see ipa_apply)
uint8_t digit_code(int e0, int e1) {
  if (e0 == 0) return e1 == 0 ? 0 : e1 > 0 ? 3 : 4;
  if (e1 == 0) return e0 > 0 ? 1 : 2;
  if (e0 == e1) return e0 > 0 ? 5 : 6;
  return e0 > 0 ? 7 : 8;
}

// a, b canonical (8 words each) -> the plan of a L + b R
IpaPlan make_plan(const uint32_t* a, const uint32_t* b) {
  IpaPlan plan;
  memset(&plan, 0, sizeof plan);
  for (int s = 0; s < 2; s++) {
    uint32_t k1[5], k2[5];
    int n1, n2;
    glv_decompose<GlvConst<IpFq>>(s ? b : a, k1, &n1, k2, &n2);
    int8_t u0[IPA_MAX_DIG], u1[IPA_MAX_DIG];
    const int len = jsf(k1, k2, u0, u1);
    for (int j = 0; j < len; j++)
      plan.dig[j] |= (uint8_t)(digit_code(n1 ? -u0[j] : u0[j], n2 ? -u1[j] : u1[j]) << (4 * s));
    plan.ndig = std::max<uint32_t>(plan.ndig, (uint32_t)len);
  }
  return plan;
}

bool overlap(const void* a, size_t an, const void* b, size_t bn) {
  if (!a || !b || !an || !bn) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bn && y < x + an;
}

void fold(zkp_ctx* ctx, const uint64_t* l_xy, const uint8_t* l_inf, const uint64_t* r_xy, const uint8_t* r_inf, size_t n,
          const uint64_t* a_host, const uint64_t* b_host, uint64_t* out_xy, uint8_t* out_inf) {
  using T = IpaLds<IpF>;
  if (n == 0) return;
  ZKP_REQUIRE(n <= ((size_t)1 << 31), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE((((uintptr_t)l_xy | (uintptr_t)r_xy | (uintptr_t)out_xy) & 15) == 0, ZKP_ERR_BAD_ARG);   // 16-B vector loads
  // in place: out_xy == l_xy or r_xy, out_inf == l_inf or r_inf; any other overlap of an output with anything is refused
  const size_t xb = n * Affine<IpF>::BYTES;
  ZKP_REQUIRE(out_xy == l_xy || !overlap(out_xy, xb, l_xy, xb), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(out_xy == r_xy || !overlap(out_xy, xb, r_xy, xb), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(out_inf == l_inf || !overlap(out_inf, n, l_inf, n), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(out_inf == r_inf || !overlap(out_inf, n, r_inf, n), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!overlap(out_xy, xb, out_inf, n) && !overlap(out_xy, xb, l_inf, n) && !overlap(out_xy, xb, r_inf, n), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(!overlap(out_inf, n, l_xy, xb) && !overlap(out_inf, n, r_xy, xb), ZKP_ERR_BAD_ARG);
  // a, b: reduced Montgomery Fr values
  const hostf::HostField fr = hostf::fr_field(IP_CURVE);
  hostf::FrE am{}, bm{};
  memcpy(am.data(), a_host, 32);
  memcpy(bm.data(), b_host, 32);
  ZKP_REQUIRE(!fr.geq(am.data()) && !fr.geq(bm.data()), ZKP_ERR_BAD_ARG);
  const hostf::FrE ac = fr.to_canonical(am), bc = fr.to_canonical(bm);
  const IpaPlan plan = make_plan(ac.data(), bc.data());
  hipStream_t st = ctx->cur->stream;
  hipLaunchKernelGGL(ipa_fold_kernel<IpF>, dim3((unsigned)((n + IPA_LANES - 1) / IPA_LANES)), dim3(IPA_LANES), IPA_LANES * T::STRIDE,
                     st, reinterpret_cast<const uint32_t*>(l_xy), l_inf, reinterpret_cast<const uint32_t*>(r_xy), r_inf, (uint32_t)n,
                     plan, reinterpret_cast<uint32_t*>(out_xy), out_inf);
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipStreamSynchronize(st));
}

const IpaVtbl kVtbl = {fold};

}  // namespace ipa_c<curve>

const IpaVtbl* ZKP_IP_SYM(ipa_vtbl_c, ZKP_CFG_CURVE)() { return &ZKP_IP_SYM(ipa_c, ZKP_CFG_CURVE)::kVtbl; }

}  // namespace zkp
