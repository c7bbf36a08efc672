// The Fr work of the Bulletproofs R1CS prover (bulletproofs/src/arithmetic_circuit.rs:305-612, inner_product_proof.rs:22-111).
// Fr only, so one object serves both curves.
//
// Ownership.  A pass over n indices runs T = BP_THREADS * min(ceil(n / BP_THREADS), BP_MAX_GROUPS) threads; thread j owns the indices
// j, j + T, ..., so a wavefront's 16-byte accesses are consecutive.  A thread forms base^j once and steps it by base^T.  The host
// supplies base^(2^b) for every bit b of j (j < 2^17) and base^T as kernel arguments: the thread multiplies the table entries of
// its set bits, one product per set bit and no squaring on the device (bits 6 and up are the same for a whole wavefront, so an
// unset one costs nothing).  0^0 = 1, so ratio 0 gives [first, 0, ...].
// The scalars of a call (one inversion, the bit tables, a few powers) are prepared on the host with 64-bit limbs (Fr64 below):
// HostField's 32-bit limbs, made for a handful of products per proof, cost more than the kernels at Bulletproofs' sizes.
//
// l(X), r(X).  With the diagonal WL, WR, WO of :436-445 written out the coefficient vectors of :471-489 are, for i < N,
//   l2 = aL + U, l3 = aO, l4 = w, l5 = sL;  r0 = -v, r1 = zn^2 Z - Y, r2 = Y aR + Z, r5 = Y sR
// with Y = y^i, Z = z^(i+1) below n and 0 from n on, zn = z^n and U = zn Z / Y, one progression of ratio z / y from zn z.  Both
// kernels form them in registers from the seven inputs; no coefficient vector is stored.  t_coeffs multiplies them into the nine
// sums of VecPoly5::special_inner_product; lr_eval evaluates both polynomials at x, writes them and sums their product.  Every
// workgroup leaves one partial per sum through fr_block_sum (nine accumulators: three groups of BP_SUM_GROUP through one buffer);
// a second launch adds the partials with one workgroup per sum.  Separate launches on one stream: no kernel waits for another
// workgroup.  Field addition is exact and every element written is canonical, so the blocking does not change a bit.
//
// The a / b fold.  a'[j] = x a[j] + x^-1 a[j + m], b'[j] = x^-1 b[j] + x b[j + m] in place for j < m = n / 2.  A thread owns the
// pair j, j + m/2 (j < m/2): it reads a and b at j, j + m/2, j + m, j + m + m/2, writes the first two, and has both factors of
// a'[j] b'[j + m/2] (cL of the next round) and a'[j + m/2] b'[j] (cR) in registers.  No other thread touches these positions.
#include <algorithm>
#include <array>
#include <cstring>

#include "bulletproofs.hpp"
#include "fr_dev.hpp"

namespace zkp {

namespace {

constexpr int BT = (int)BP_THREADS;
constexpr int SG = (int)BP_SUM_GROUP;
constexpr int NT_COEFF = 9;                                      // t2 .. t10
static_assert(NT_COEFF % SG == 0, "the sums are reduced in whole groups");

constexpr int JB = 17;                                           // bits of a thread's first index
static_assert(((size_t)1 << JB) == (size_t)BP_THREADS * BP_MAX_GROUPS, "one table entry per bit of the largest thread index");
// the scalars of the l(X), r(X) kernels; S_YB, S_ZB, S_QB: y^(2^b), z^(2^b), (z / y)^(2^b) for b < JB
enum { S_YT, S_ZT, S_QT, S_ZN2, S_U0, S_X, S_X2, S_X5, S_YB, S_ZB = S_YB + JB, S_QB = S_ZB + JB, S_COUNT = S_QB + JB };
enum { P_FIRST, P_STEP, P_BITS, P_COUNT = P_BITS + JB };         // the scalars of powers_kernel

struct BpVecs {
  const uint32_t *aL, *aR, *aO, *w, *v, *sL, *sR;
  size_t n, n_w, n_s, N;
};

template <class P>
__global__ __launch_bounds__(BT) void powers_kernel(FrArgs<Fp<P>, P_COUNT> c, uint32_t* __restrict__ out, size_t n) {
  using F = Fp<P>;
  const size_t T = (size_t)gridDim.x * BT;
  const size_t j = (size_t)blockIdx.x * BT + threadIdx.x;
  if (j >= n) return;
  F x = c.get(P_FIRST);
#pragma unroll 1
  for (int b = 0; b < JB; b++)
    if ((j >> b) & 1) x = x * c.get(P_BITS + b);
  if (j + T >= n) {                                              // the only index: no step
    x.store(out + j * 8);
    return;
  }
  const F step = c.get(P_STEP);
  for (size_t i = j; i < n; i += T) {
    x.store(out + i * 8);
    x = x * step;
  }
}

// The coefficients of index i.  Y, Zp = z^(i+1) and U are the thread's running powers; Zp and U count only below n.
template <class F>
struct Coeffs {
  F l2, l3, l4, l5, r0, r1, r2, r5;
  __device__ __forceinline__ Coeffs(const BpVecs& b, size_t i, const F& Y, const F& Zp, const F& U, const F& zn2) {
    const bool in_n = i < b.n, in_w = i < b.n_w, in_s = i < b.n_s;
    const F Z = in_n ? Zp : F::zero();
    l2 = in_n ? F::load(b.aL + i * 8) + U : F::zero();
    l3 = in_n ? F::load(b.aO + i * 8) : F::zero();
    l4 = in_w ? F::load(b.w + i * 8) : F::zero();
    l5 = in_s ? F::load(b.sL + i * 8) : F::zero();
    r0 = in_w ? F::load(b.v + i * 8).neg() : F::zero();
    r1 = in_n ? zn2 * Z - Y : Y.neg();
    r2 = in_n ? Y * F::load(b.aR + i * 8) + Z : F::zero();
    r5 = in_s ? Y * F::load(b.sR + i * 8) : F::zero();
  }
};

// the thread's powers at its first index j (from the bit tables) and their steps
template <class F>
struct Powers {
  F Y, Zp, U, yT, zT, qT;
  __device__ __forceinline__ Powers(const FrArgs<F, S_COUNT>& c, size_t j) {
    Y = F::one();
    Zp = c.get(S_ZB);                                            // z^(j+1) = z z^j
    U = c.get(S_U0);
#pragma unroll 1
    for (int b = 0; b < JB; b++) {
      if ((j >> b) & 1) {                                        // three independent products
        Y = Y * c.get(S_YB + b);
        Zp = Zp * c.get(S_ZB + b);
        U = U * c.get(S_QB + b);
      }
    }
    yT = c.get(S_YT);
    zT = c.get(S_ZT);
    qT = c.get(S_QT);
  }
  // more: the thread owns a further index; in_n: that index is below n (from n on neither Zp nor U is read again)
  __device__ __forceinline__ void step(bool more, bool in_n) {
    if (!more) return;
    Y = Y * yT;
    if (in_n) {
      Zp = Zp * zT;
      U = U * qT;
    }
  }
};

// partial[k * gridDim.x + block] = the block's share of t_(k+2)
template <class P>
__global__ __launch_bounds__(BT) void t_coeffs_kernel(BpVecs b, FrArgs<Fp<P>, S_COUNT> c, uint32_t* __restrict__ partial) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[SG * BT * 32];
  const size_t T = (size_t)gridDim.x * BT;
  const size_t j = (size_t)blockIdx.x * BT + threadIdx.x;
  F t[NT_COEFF];
#pragma unroll
  for (int k = 0; k < NT_COEFF; k++) t[k] = F::zero();
  if (j < b.N) {
    Powers<F> pw(c, j);
    const F zn2 = c.get(S_ZN2);
    for (size_t i = j; i < b.N; i += T) {
      const Coeffs<F> q(b, i, pw.Y, pw.Zp, pw.U, zn2);
      t[0] = t[0] + q.l2 * q.r0;
      t[1] = t[1] + q.l2 * q.r1 + q.l3 * q.r0;
      t[2] = t[2] + q.l2 * q.r2 + q.l3 * q.r1 + q.l4 * q.r0;
      t[3] = t[3] + q.l3 * q.r2 + q.l4 * q.r1 + q.l5 * q.r0;
      t[4] = t[4] + q.l4 * q.r2 + q.l5 * q.r1;
      t[5] = t[5] + q.l2 * q.r5 + q.l5 * q.r2;
      t[6] = t[6] + q.l3 * q.r5;
      t[7] = t[7] + q.l4 * q.r5;
      t[8] = t[8] + q.l5 * q.r5;
      pw.step(i + T < b.N, i + T < b.n);
    }
  }
#pragma unroll
  for (int g = 0; g < NT_COEFF; g += SG) {
    F acc[SG];
#pragma unroll
    for (int k = 0; k < SG; k++) acc[k] = t[g + k];
    fr_block_sum<F, BT, SG>(acc, smem);                          // ends on a barrier: the next group reuses smem
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < SG; k++) acc[k].store(partial + ((size_t)(g + k) * gridDim.x + blockIdx.x) * 8);
    }
  }
}

// l_x, r_x written for i < N; partial[block] = the block's share of <l_x, r_x>
template <class P>
__global__ __launch_bounds__(BT) void lr_eval_kernel(BpVecs b, FrArgs<Fp<P>, S_COUNT> c, uint32_t* __restrict__ l_x,
                                                     uint32_t* __restrict__ r_x, uint32_t* __restrict__ partial) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[BT * 32];
  const size_t T = (size_t)gridDim.x * BT;
  const size_t j = (size_t)blockIdx.x * BT + threadIdx.x;
  F acc[1] = {F::zero()};
  if (j < b.N) {
    Powers<F> pw(c, j);
    const F zn2 = c.get(S_ZN2), x = c.get(S_X), x2 = c.get(S_X2), x5 = c.get(S_X5);
    for (size_t i = j; i < b.N; i += T) {
      const Coeffs<F> q(b, i, pw.Y, pw.Zp, pw.U, zn2);
      const F l = x2 * (q.l2 + x * (q.l3 + x * (q.l4 + x * q.l5)));
      const F r = q.r0 + x * q.r1 + x2 * q.r2 + x5 * q.r5;
      l.store(l_x + i * 8);
      r.store(r_x + i * 8);
      acc[0] = acc[0] + l * r;
      pw.step(i + T < b.N, i + T < b.n);
    }
  }
  fr_block_sum<F, BT, 1>(acc, smem);
  if (threadIdx.x == 0) acc[0].store(partial + (size_t)blockIdx.x * 8);
}

// h = m / 2 pairs (h == 0: m == 1, the single element).  want_c: partial[block], partial[gridDim.x + block] = the block's
// shares of cL and cR.
template <class P>
__global__ __launch_bounds__(BT) void fold_ab_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, size_t m, FrArgs<Fp<P>, 2> c,
                                                     int want_c, uint32_t* __restrict__ partial) {
  using F = Fp<P>;
  __shared__ __attribute__((aligned(16))) char smem[2 * BT * 32];
  const F x = c.get(0), xi = c.get(1);
  const size_t h = m / 2;
  const size_t T = (size_t)gridDim.x * BT;
  const size_t j = (size_t)blockIdx.x * BT + threadIdx.x;
  if (h == 0) {                                                  // one workgroup, the same branch for all of it
    if (j == 0) {
      (x * F::load(a) + xi * F::load(a + 8)).store(a);
      (xi * F::load(b) + x * F::load(b + 8)).store(b);
    }
    return;
  }
  F acc[2] = {F::zero(), F::zero()};
  for (size_t p = j; p < h; p += T) {
    const F a_lo = x * F::load(a + p * 8) + xi * F::load(a + (p + m) * 8);
    const F a_hi = x * F::load(a + (p + h) * 8) + xi * F::load(a + (p + h + m) * 8);
    const F b_lo = xi * F::load(b + p * 8) + x * F::load(b + (p + m) * 8);
    const F b_hi = xi * F::load(b + (p + h) * 8) + x * F::load(b + (p + h + m) * 8);
    a_lo.store(a + p * 8);
    a_hi.store(a + (p + h) * 8);
    b_lo.store(b + p * 8);
    b_hi.store(b + (p + h) * 8);
    if (want_c) {
      acc[0] = acc[0] + a_lo * b_hi;
      acc[1] = acc[1] + a_hi * b_lo;
    }
  }
  if (!want_c) return;                                           // a kernel argument: the same for every thread
  fr_block_sum<F, BT, 2>(acc, smem);
  if (threadIdx.x == 0) {
    acc[0].store(partial + (size_t)blockIdx.x * 8);
    acc[1].store(partial + ((size_t)gridDim.x + blockIdx.x) * 8);
  }
}

uint32_t groups_for(size_t n) { return (uint32_t)std::min<size_t>(std::max<size_t>((n + BT - 1) / BT, 1), BP_MAX_GROUPS); }

// Host Montgomery arithmetic on four 64-bit limbs, R = 2^256: the words of HostField and of the device, so values pass between
// them as they are.
struct Fr64 {
  using E = std::array<uint64_t, 4>;
  typedef unsigned __int128 u128;
  uint64_t m[4], ninv;                                           // the modulus, -1 / modulus mod 2^64
  E one;
  uint32_t pm2[8];
  explicit Fr64(int curve) {
    const hostf::HostField f = hostf::fr_field(curve);
    for (int i = 0; i < 4; i++) m[i] = f.mod[2 * i] | (uint64_t)f.mod[2 * i + 1] << 32;
    uint64_t x = 1;
    for (int k = 0; k < 6; k++) x *= 2 - m[0] * x;               // Newton: 1 / m[0] mod 2^64
    ninv = 0 - x;
    memcpy(one.data(), f.one, 32);
    memcpy(pm2, f.pm2, 32);
  }
  static E load(const uint64_t* host) {
    E e;
    memcpy(e.data(), host, 32);
    return e;
  }
  bool geq(const uint64_t* t) const {
    for (int i = 3; i >= 0; i--)
      if (t[i] != m[i]) return t[i] > m[i];
    return true;
  }
  E mul(const E& a, const E& b) const {
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
      u128 c = 0;
      for (int j = 0; j < 4; j++) {
        c += (u128)a[j] * b[i] + t[j];
        t[j] = (uint64_t)c;
        c >>= 64;
      }
      c += t[4];
      t[4] = (uint64_t)c;
      t[5] = (uint64_t)(c >> 64);
      const uint64_t q = t[0] * ninv;
      c = ((u128)q * m[0] + t[0]) >> 64;
      for (int j = 1; j < 4; j++) {
        c += (u128)q * m[j] + t[j];
        t[j - 1] = (uint64_t)c;
        c >>= 64;
      }
      c += t[4];
      t[3] = (uint64_t)c;
      t[4] = t[5] + (uint64_t)(c >> 64);
    }
    if (t[4] || geq(t)) {
      u128 br = 0;
      for (int i = 0; i < 4; i++) {
        const u128 d = (u128)t[i] - m[i] - br;
        t[i] = (uint64_t)d;
        br = (d >> 64) & 1;
      }
    }
    return {t[0], t[1], t[2], t[3]};
  }
  E pow(E a, uint64_t e) const {
    E r = one;
    for (; e; e >>= 1) {
      if (e & 1) r = mul(r, a);
      a = mul(a, a);
    }
    return r;
  }
  E inverse(const E& a) const {                                  // Fermat: a^(r - 2)
    E r = one;
    for (int bit = 255; bit >= 0; bit--) {
      r = mul(r, r);
      if ((pm2[bit >> 5] >> (bit & 31)) & 1) r = mul(r, a);
    }
    return r;
  }
};

// base^(2^b) for b < JB into c[first ..]
template <class Pack>
void set_bit_powers(Pack& c, int first, const Fr64& fr, Fr64::E base) {
  for (int b = 0; b < JB; b++) {
    c.set(first + b, base.data());
    base = fr.mul(base, base);
  }
}

// the rules of zkp_bp_vectors; returns the kernels' view of it
BpVecs require_vectors(const zkp_bp_vectors* vecs) {
  ZKP_REQUIRE(vecs != nullptr, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(is_pow2(vecs->N) && vecs->N <= ((size_t)1 << BP_MAX_LOG), ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(vecs->n <= vecs->N && vecs->n_w <= vecs->N && vecs->n_s <= vecs->N, ZKP_ERR_BAD_ARG);
  const struct {
    const uint64_t* p;
    size_t len;
  } all[7] = {{vecs->aL, vecs->n},  {vecs->aR, vecs->n},   {vecs->aO, vecs->n},  {vecs->w, vecs->n_w},
              {vecs->v, vecs->n_w}, {vecs->sL, vecs->n_s}, {vecs->sR, vecs->n_s}};
  for (const auto& e : all) {
    if (e.len == 0) continue;                                    // never read: the pointer may be NULL
    ZKP_REQUIRE(e.p != nullptr, ZKP_ERR_BAD_ARG);
    require_aligned16(e.p);
  }
  auto w32 = [](const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); };
  return {w32(vecs->aL), w32(vecs->aR), w32(vecs->aO), w32(vecs->w), w32(vecs->v), w32(vecs->sL), w32(vecs->sR),
          vecs->n,       vecs->n_w,     vecs->n_s,     vecs->N};
}

// y != 0, y and z below r; the scalars both l(X), r(X) kernels read, for T threads
template <class F>
FrArgs<F, S_COUNT> lr_scalars(const Fr64& fr, const BpVecs& b, const uint64_t* y_host, const uint64_t* z_host, uint64_t T) {
  const Fr64::E y = Fr64::load(y_host), z = Fr64::load(z_host);
  const Fr64::E q = fr.mul(z, fr.inverse(y)), zn = fr.pow(z, b.n);
  FrArgs<F, S_COUNT> c{};
  c.set(S_YT, fr.pow(y, T).data());
  c.set(S_ZT, fr.pow(z, T).data());
  c.set(S_QT, fr.pow(q, T).data());
  c.set(S_ZN2, fr.mul(zn, zn).data());
  c.set(S_U0, fr.mul(zn, z).data());
  set_bit_powers(c, S_YB, fr, y);
  set_bit_powers(c, S_ZB, fr, z);
  set_bit_powers(c, S_QB, fr, q);
  return c;
}

void require_yz(int curve, const uint64_t* y_host, const uint64_t* z_host) {
  ZKP_REQUIRE(y_host && z_host, ZKP_ERR_BAD_ARG);
  fr_require_canonical(curve, y_host, 1);
  fr_require_canonical(curve, z_host, 1);
  ZKP_REQUIRE(y_host[0] | y_host[1] | y_host[2] | y_host[3], ZKP_ERR_BAD_ARG);
}

}  // namespace

void fr_powers(zkp_ctx* ctx, int curve, const uint64_t* first_host, const uint64_t* ratio_host, uint64_t* out_dev, size_t n) {
  fr_require_curve(curve);
  if (n == 0) return;
  ZKP_REQUIRE(first_host && ratio_host && out_dev, ZKP_ERR_BAD_ARG);
  require_aligned16(out_dev);
  ZKP_REQUIRE(n <= ((size_t)1 << BP_MAX_LOG), ZKP_ERR_BAD_ARG);
  fr_require_canonical(curve, first_host, 1);
  fr_require_canonical(curve, ratio_host, 1);
  const uint32_t nwg = groups_for(n);
  const Fr64 fr(curve);
  const Fr64::E ratio = Fr64::load(ratio_host);
  hipStream_t st = ctx->cur->stream;
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    FrArgs<Fp<P>, P_COUNT> c{};
    c.set(P_FIRST, first_host);
    c.set(P_STEP, fr.pow(ratio, (uint64_t)nwg * BT).data());
    set_bit_powers(c, P_BITS, fr, ratio);
    hipLaunchKernelGGL(powers_kernel<P>, dim3(nwg), dim3(BT), 0, st, c, reinterpret_cast<uint32_t*>(out_dev), n);
  });
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipStreamSynchronize(st));
}

void fr_bp_t_coeffs(zkp_ctx* ctx, int curve, const zkp_bp_vectors* vecs, const uint64_t* y_host, const uint64_t* z_host,
                    uint64_t* t_out_host) {
  fr_require_curve(curve);
  ZKP_REQUIRE(t_out_host != nullptr, ZKP_ERR_BAD_ARG);
  const BpVecs b = require_vectors(vecs);
  require_yz(curve, y_host, z_host);
  const uint32_t nwg = groups_for(b.N);
  hipStream_t st = ctx->cur->stream;
  Scratch sc;
  const size_t o_out = sc.take(NT_COEFF * 32), o_part = sc.take((size_t)NT_COEFF * nwg * 32);
  sc.resolve(ctx->poly_tmp);
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    const auto c = lr_scalars<Fp<P>>(Fr64(curve), b, y_host, z_host, (uint64_t)nwg * BT);
    hipLaunchKernelGGL(t_coeffs_kernel<P>, dim3(nwg), dim3(BT), 0, st, b, c, sc.at<uint32_t>(o_part));
    fr_sum_partials<P, BT>(st, sc.at<uint32_t>(o_part), nwg, NT_COEFF, sc.at<uint32_t>(o_out));
  });
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipMemcpyAsync(t_out_host, sc.at<uint32_t>(o_out), NT_COEFF * 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

void fr_bp_lr_eval(zkp_ctx* ctx, int curve, const zkp_bp_vectors* vecs, const uint64_t* y_host, const uint64_t* z_host,
                   const uint64_t* x_host, uint64_t* l_x_dev, uint64_t* r_x_dev, uint64_t* t_x_out_host) {
  fr_require_curve(curve);
  ZKP_REQUIRE(x_host && l_x_dev && r_x_dev && t_x_out_host, ZKP_ERR_BAD_ARG);
  const BpVecs b = require_vectors(vecs);
  require_yz(curve, y_host, z_host);
  fr_require_canonical(curve, x_host, 1);
  require_aligned16(l_x_dev);
  require_aligned16(r_x_dev);
  require_disjoint_outputs({fr_span(l_x_dev, b.N, true), fr_span(r_x_dev, b.N, true), fr_span(b.aL, b.n, false),
                            fr_span(b.aR, b.n, false), fr_span(b.aO, b.n, false), fr_span(b.w, b.n_w, false),
                            fr_span(b.v, b.n_w, false), fr_span(b.sL, b.n_s, false), fr_span(b.sR, b.n_s, false)});   // length 0: never read
  const uint32_t nwg = groups_for(b.N);
  hipStream_t st = ctx->cur->stream;
  Scratch sc;
  const size_t o_out = sc.take(32), o_part = sc.take((size_t)nwg * 32);
  sc.resolve(ctx->poly_tmp);
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    const Fr64 fr(curve);
    const Fr64::E x = Fr64::load(x_host), x2 = fr.mul(x, x);
    auto c = lr_scalars<Fp<P>>(fr, b, y_host, z_host, (uint64_t)nwg * BT);
    c.set(S_X, x.data());
    c.set(S_X2, x2.data());
    c.set(S_X5, fr.mul(fr.mul(x2, x2), x).data());
    hipLaunchKernelGGL(lr_eval_kernel<P>, dim3(nwg), dim3(BT), 0, st, b, c, reinterpret_cast<uint32_t*>(l_x_dev),
                       reinterpret_cast<uint32_t*>(r_x_dev), sc.at<uint32_t>(o_part));
    fr_sum_partials<P, BT>(st, sc.at<uint32_t>(o_part), nwg, 1, sc.at<uint32_t>(o_out));
  });
  ZKP_HIP(hipGetLastError());
  ZKP_HIP(hipMemcpyAsync(t_x_out_host, sc.at<uint32_t>(o_out), 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

void fr_ipa_fold_ab(zkp_ctx* ctx, int curve, uint64_t* a_dev, uint64_t* b_dev, size_t n, const uint64_t* x_host, uint64_t* c_out_host) {
  fr_require_curve(curve);
  ZKP_REQUIRE(a_dev && b_dev && x_host, ZKP_ERR_BAD_ARG);
  require_aligned16(a_dev);
  require_aligned16(b_dev);
  ZKP_REQUIRE(is_pow2(n) && n >= 2 && n <= ((size_t)1 << BP_MAX_LOG), ZKP_ERR_BAD_ARG);
  require_disjoint_outputs({fr_span(a_dev, n, true), fr_span(b_dev, n, true)});
  fr_require_canonical(curve, x_host, 1);
  ZKP_REQUIRE(x_host[0] | x_host[1] | x_host[2] | x_host[3], ZKP_ERR_BAD_ARG);
  const size_t m = n / 2;
  const bool want_c = c_out_host != nullptr && m >= 2;
  const uint32_t nwg = groups_for(m / 2);
  const Fr64::E xi = Fr64(curve).inverse(Fr64::load(x_host));
  hipStream_t st = ctx->cur->stream;
  Scratch sc;
  const size_t o_out = sc.take(2 * 32), o_part = sc.take((size_t)2 * nwg * 32);
  if (want_c) sc.resolve(ctx->poly_tmp);
  uint32_t* d_part = want_c ? sc.at<uint32_t>(o_part) : nullptr;
  with_fr(curve, [&](auto tag) {
    using P = decltype(tag);
    FrArgs<Fp<P>, 2> c{};
    c.set(0, x_host);
    c.set(1, xi.data());
    hipLaunchKernelGGL(fold_ab_kernel<P>, dim3(nwg), dim3(BT), 0, st, reinterpret_cast<uint32_t*>(a_dev), reinterpret_cast<uint32_t*>(b_dev), m,
                       c, want_c ? 1 : 0, d_part);
    if (want_c) fr_sum_partials<P, BT>(st, d_part, nwg, 2, sc.at<uint32_t>(o_out));
  });
  ZKP_HIP(hipGetLastError());
  if (want_c) ZKP_HIP(hipMemcpyAsync(c_out_host, sc.at<uint32_t>(o_out), 2 * 32, hipMemcpyDeviceToHost, st));
  ZKP_HIP(hipStreamSynchronize(st));
}

}  // namespace zkp
