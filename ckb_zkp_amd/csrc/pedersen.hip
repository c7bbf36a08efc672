// Resident Pedersen key (zkp_pedersen_key_*), row commitments (zkp_pedersen_commit_rows_dev) and the Fr vector-matrix product
// (zkp_fr_vecmat_dev): `packing_poly_commit` / `poly_commit_vec` (spartan/src/commitments.rs:10-56, libra/src/evaluate.rs:130-170)
// and the row fold of LogDotProductProof::reduce_prover (hyrax/src/commitment.rs:335-578).  Compiled once per curve, G1 only:
// -DZKP_CFG_CURVE={0,1}.
//
// The key: window tables T[w][j] = 2^(c w) g_j for w < W, j <= n_gens (h is generator n_gens), affine Montgomery points, level w
// at table + w (n_gens + 1) points, plus one identity flag per generator (an identity stays one at every level and is stored as
// (0, 0)).  Affine halves the bytes a (generator, window) pair gathers (64 / 96 B against the 144 / 224 B of a BkPoint); the batch
// inversion it needs per level is the affine pass below, so creation is 2 W launches over one BkPoint per generator:
// level w -> affine, then c doublings in registers.
//
// A commitment of `rows` rows is three launches whatever rows and cols are:
//   launch 1  one wave per (row, slice of <= G generators), all W windows at once; the wave owns 2^(c-1) XYZZ buckets in LDS:
//             a. digits: a lane owns generators t, t + 64, ... of the slice, reads each scalar once (32 B, from_mont fused), walks
//                DigitIter::next over the W windows once and emits W entries (bucket, sign) at q = e W + w; zero digits and
//                identity generators go to the sentinel key nb;
//             b. - d. the stable LDS counting sort, the per-lane chunks and the boundary-slot tree of small_bucket_kernel
//                (msm_small.hip) over the <= 4096 entries; entry q stages table point T[q % W][slice + q / W];
//             e. sum_b (b + 1) B_b as there.  There is no window weight left to apply: the tables carry it.
//   launch 2  one wave per row: lane t adds slices t, t + 64, ... into its LDS slot, lane w < W adds the blind term's window w —
//             d_w T[w][h] by double-and-add over the c bits of |d_w| in registers — and an LDS tree adds the 64 slots;
//   launch 3  one lane per row: Montgomery's trick per workgroup over d = ZZ ZZZ as in ipa.hip (product tree in LDS, one Fermat
//             inversion per 64 rows, identities kept out of the tree), canonical affine output.
// Every addition is BkPoint::add / add_mem (bucket_dev.hpp): complete, so equal and opposite generators, identities and a row that
// sums to the identity need no special path.  Every output is the canonical affine form, so the result is bit-exact whatever the
// order of the additions.
//
// zkp_fr_vecmat_dev: out[j] = sum_i l[i] m[i cols + j].  Lanes take consecutive columns (a row of 64 x 32 B is one 2 KiB burst),
// a workgroup takes VECMAT_ROW_CHUNK rows; with more than one chunk the partial sums go to the arena and a second launch adds them
// chunk by chunk.  Field addition is exact, so the split does not change a bit of the result.
#include <vector>

#include "bucket_dev.hpp"
#include "ec_dev.hpp"
#include "fr_dev.hpp"
#include "msm_digits.hpp"
#include "msm_small.hpp"
#include "pedersen.hpp"

#ifndef ZKP_CFG_CURVE
#error "compile with -DZKP_CFG_CURVE=0|1"
#endif

// the handle of include/zkp_accel.h; the same definition in both per-curve objects
struct zkp_pedersen_key {
  int curve = 0;
  zkp_ctx* ctx = nullptr;
  uint32_t n_gens = 0;
  uint32_t* table = nullptr;     // W levels of n_gens + 1 affine Montgomery points (device)
  uint8_t* inf = nullptr;        // n_gens + 1 identity flags (device)
  size_t table_bytes = 0;
};

namespace zkp {

static_assert(PED_LDS_MAX == SMALL_LDS_MAX && PED_LANES == SMALL_LANES, "the bucket pass is sized like msm_small");
static_assert(PED_MAX_GENS == ZKP_PEDERSEN_MAX_GENS && PED_MAX_GENS == ZKP_MSM_SMALL_MAX_G1, "the header quotes the same cap");
static_assert(VECMAT_ROW_CHUNK == ZKP_FR_VECMAT_ROW_CHUNK, "the header quotes the same chunk");

#if ZKP_CFG_CURVE == 0
using PdFq = Bn254Fq;
using PdFr = Bn254Fr;
constexpr int PD_CURVE = ZKP_BN254;
#else
using PdFq = Bls381Fq;
using PdFr = Bls381Fr;
constexpr int PD_CURVE = ZKP_BLS12_381;
#endif
using PdF = Fp<PdFq>;
constexpr int PD_C = pedersen_c(ZKP_CFG_CURVE);
constexpr int PD_W = (256 + PD_C) / PD_C;
static_assert(pedersen_bk_bytes(ZKP_CFG_CURVE) == (uint32_t)BkPoint<PdF>::BYTES, "pedersen.hpp sizes the LDS with this");
static_assert(PD_W * PD_C > 256 && PD_W <= PED_LANES, "the top window absorbs the last carry; one lane per window of the blind term");
static_assert((1 << (PD_C - 1)) % PED_LANES == 0, "the bucket fold gives every lane the same number of buckets");

#define ZKP_PD_CAT(a, b) a##b
#define ZKP_PD_SYM(name, cu) ZKP_PD_CAT(name, cu)
// the same source is compiled twice: one namespace per curve
namespace ZKP_PD_SYM(pedersen_c, ZKP_CFG_CURVE) {

constexpr uint32_t SLOT_EMPTY = 0xffffu;       // key of a boundary slot that holds nothing (above every bucket index)

template <int BY>
__device__ __forceinline__ void pd_zero(char* p) {
  uint32_t* w = reinterpret_cast<uint32_t*>(p);
#pragma unroll
  for (int i = 0; i < BY / 4; i++) w[i] = 0;
}
// table point `idx` (negated for a negative digit) -> BkPoint layout at out; never an identity (those take the sentinel key)
template <class F>
__device__ __forceinline__ void pd_stage(const uint32_t* table, size_t idx, bool neg, char* out) {
  Affine<F> a = Affine<F>::load(table + idx * (Affine<F>::BYTES / 4));
  if (neg) a.y = a.y.neg();
  BkPoint<F>::from_sat(XYZZ<F>::from_affine(a)).store(out);
}

// launch 1: workgroup row * S + j -> partial[row * S + j]
template <class F, class FrP, int C, int W>
__global__ __launch_bounds__(PED_LANES) void ped_bucket_kernel(const uint32_t* __restrict__ table, const uint8_t* __restrict__ ginf,
                                                               uint32_t nt, const uint32_t* __restrict__ scalars, uint32_t cols,
                                                               uint32_t S, uint32_t g, uint32_t emax, char* __restrict__ partial) {
  using B = BkPoint<F>;
  constexpr int BY = B::BYTES;
  constexpr uint32_t nb = 1u << (C - 1);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const uint32_t row = blockIdx.x / S, j = blockIdx.x % S;
  const uint32_t p0 = j * g, m = p0 < cols ? min(g, cols - p0) : 0u;
  const uint32_t M = min(m * (uint32_t)W, emax);                 // entries of this slice (m W <= emax by the plan)

  char* bk = smem;                                               // nb buckets
  char* slots = bk + (size_t)nb * BY;                            // 2 boundary slots per lane
  char* stage = slots + PED_SLOTS * BY;                          // one staged point per lane
  uint32_t* skey = reinterpret_cast<uint32_t*>(stage + PED_LANES * BY);      // PED_SLOTS keys
  uint32_t* hist = skey + PED_SLOTS;                             // nb + 1 counts -> offsets -> cursors
  uint32_t* srt = hist + nb + 4;                                 // sorted entries: key << 16 | negative << 15 | entry index
  uint16_t* ent = reinterpret_cast<uint16_t*>(srt + emax);       // digit of each entry: key | negative << 15

  for (uint32_t q = t; q < nb * (BY / 4); q += PED_LANES) reinterpret_cast<uint32_t*>(bk)[q] = 0;
  for (uint32_t q = t; q <= nb; q += PED_LANES) hist[q] = 0;
  __syncthreads();

  // a. all W digits of every generator of the slice
  for (uint32_t e = t; e < m && (e + 1) * W <= M; e += PED_LANES) {
    const uint32_t gi = p0 + e;
    const bool id = ginf[gi] != 0;
    DigitIter it;
    if (!id) it = load_scalar<FrP>(scalars, (size_t)row * cols + gi, 1);
    for (int w = 0; w < W; w++) {
      uint32_t key = nb, neg = 0;
      if (!id) {
        it.next(w, C, W, nb, key, neg);
        if (key == nb) neg = 0;
      }
      ent[e * W + w] = (uint16_t)(key | neg << 15);
      atomicAdd(&hist[key], 1u);
    }
  }
  __syncthreads();
  {                                                              // exclusive scan of the nb + 1 counts
    const uint32_t nk = nb + 1, per = (nk + PED_LANES - 1) / PED_LANES;
    const uint32_t q0 = min(nk, t * per), q1 = min(nk, q0 + per);
    uint32_t loc = 0;
    for (uint32_t q = q0; q < q1; q++) loc += hist[q];
    uint32_t inc = loc;
    for (int o = 1; o < PED_LANES; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)inc, o, PED_LANES);
      if (t >= o) inc += y;
    }
    uint32_t run = inc - loc;
    for (uint32_t q = q0; q < q1; q++) {
      const uint32_t h = hist[q];
      hist[q] = run;
      run += h;
    }
  }
  __syncthreads();
  const uint32_t mp = hist[nb];                                  // entries with a non-zero digit: sorted[0, mp)
  __syncthreads();

  // b. stable scatter, 64 entries per round
  for (uint32_t r = 0; r < M; r += PED_LANES) {
    const uint32_t e = r + t;
    const bool act = e < M;
    const uint32_t v = act ? ent[e] : 0u;
    const uint32_t key = v & 0x7fffu;
    uint64_t same = __ballot(act);
    for (int b = 0; b < C; b++) {                                // keys are <= nb: C bits
      const bool bit = (key >> b) & 1;
      const uint64_t bb = __ballot(bit);
      same &= bit ? bb : ~bb;
    }
    if (act) {
      const uint32_t rank = (uint32_t)__popcll(same & ((1ull << t) - 1));
      srt[hist[key] + rank] = key << 16 | (v & 0x8000u) | e;
      if ((same >> t) == 1ull) hist[key] += (uint32_t)__popcll(same);   // the highest lane of the group advances the cursor
    }
    __syncthreads();
  }

  // c. one chunk of the sorted list per lane
  {
    const uint32_t L = (mp + PED_LANES - 1) / PED_LANES;
    const uint32_t s0 = min(mp, t * L), s1 = min(mp, s0 + L);
    char* H = slots + (size_t)(2 * t) * BY;
    char* T = H + BY;                                            // the running sum of the current run
    char* stg = stage + (size_t)t * BY;
    pd_zero<BY>(H);
    pd_zero<BY>(T);
    uint32_t hkey = SLOT_EMPTY, tkey = SLOT_EMPTY;
    if (s0 < s1) {
      uint32_t cur = srt[s0] >> 16;
      bool first = true;
      for (uint32_t q = s0; q < s1; q++) {
        const uint32_t v = srt[q], key = v >> 16;
        if (key != cur) {
          if (first) {
            B::copy_point(H, T);
            hkey = cur;
            first = false;
          } else {
            B::copy_point(bk + (size_t)cur * BY, T);             // a run strictly inside the chunk: this lane owns the bucket
          }
          pd_zero<BY>(T);
          cur = key;
        }
        const uint32_t en = v & 0x7fffu;                         // entry e W + w: generator p0 + e at level w
        pd_stage<F>(table, (size_t)(en % W) * nt + p0 + en / W, (v & 0x8000u) != 0, stg);
        B::add_mem(T, stg, T);
      }
      tkey = cur;
      if (first) hkey = cur;                                     // one run: H stays the identity under the same key
    }
    skey[2 * t] = hkey;
    skey[2 * t + 1] = tkey;
  }
  __syncthreads();

  // d. boundary runs: the slot at the right end of a block holds the sum of the block's entries with that slot's key
  for (int h = 1; h < PED_SLOTS; h <<= 1) {
    if (t < PED_SLOTS / (2 * h)) {
      const int i = t * 2 * h + h - 1, k = i + h;
      const uint32_t ki = skey[i], kk = skey[k];
      char* si = slots + (size_t)i * BY;
      if (ki == kk) {
        if (ki != SLOT_EMPTY) B::add_mem(slots + (size_t)k * BY, si, slots + (size_t)k * BY);
      } else if (ki != SLOT_EMPTY) {                             // ki < kk: block i ends its run
        B::add_mem(bk + (size_t)ki * BY, si, bk + (size_t)ki * BY);
      }
    }
    __syncthreads();
  }
  if (t == 0 && skey[PED_SLOTS - 1] != SLOT_EMPTY) {
    char* b = bk + (size_t)skey[PED_SLOTS - 1] * BY;
    B::add_mem(b, slots + (size_t)(PED_SLOTS - 1) * BY, b);
  }
  __syncthreads();

  // e. sum_b (b + 1) B_b
  constexpr int per_lane = (int)(nb / PED_LANES);
  char* R = slots + (size_t)t * BY;
  char* V = slots + (size_t)(PED_LANES + t) * BY;
  pd_zero<BY>(R);
  pd_zero<BY>(V);
  for (int b = (t + 1) * per_lane - 1; b >= t * per_lane; b--) {
    B::add_mem(R, bk + (size_t)b * BY, R);
    B::add_mem(V, R, V);                                         // V_t = sum over the lane's buckets of (b - t per_lane + 1) B_b
  }
  __syncthreads();
  char* X = slots;                                               // S_t, then its suffix sums (double-buffered in the bucket area)
  char* Y = bk;
  for (int h = 1; h < PED_LANES; h <<= 1) {
    if (t + h < PED_LANES) B::add_mem(X + (size_t)t * BY, X + (size_t)(t + h) * BY, Y + (size_t)t * BY);
    else B::copy_point(Y + (size_t)t * BY, X + (size_t)t * BY);
    __syncthreads();
    char* s = X;
    X = Y;
    Y = s;
  }
  if (t >= 1) {                                                  // sum_t t per_lane S_t = per_lane sum_{u >= 1} suffix_u
    B u = B::load(X + (size_t)t * BY);
    for (int s = 1; s < per_lane; s <<= 1) u = u.dbl();
    u.store(stage + (size_t)t * BY);
    B::add_mem(V, stage + (size_t)t * BY, V);
  }
  __syncthreads();
  for (int h = PED_LANES / 2; h > 0; h >>= 1) {
    if (t < h) B::add_mem(V, V + (size_t)h * BY, V);
    __syncthreads();
  }
  if (t == 0) B::copy_point(partial + (size_t)blockIdx.x * BY, V);
}

// launch 2: one workgroup per row -> rowsum[row]
template <class F, class FrP, int C, int W>
__global__ __launch_bounds__(PED_LANES) void ped_row_kernel(const char* __restrict__ partial, uint32_t S,
                                                            const uint32_t* __restrict__ table, const uint8_t* __restrict__ ginf,
                                                            uint32_t nt, const uint32_t* __restrict__ blinds, char* __restrict__ rowsum) {
  using B = BkPoint<F>;
  constexpr int BY = B::BYTES;
  constexpr uint32_t nb = 1u << (C - 1);
  __shared__ __attribute__((aligned(16))) char smem[2 * PED_LANES * BY];
  const int t = threadIdx.x;
  const uint32_t row = blockIdx.x;
  char* my = smem + (size_t)t * BY;
  char* stg = smem + (size_t)(PED_LANES + t) * BY;
  pd_zero<BY>(my);
  for (uint32_t j = t; j < S; j += PED_LANES) B::add_mem(my, partial + ((size_t)row * S + j) * BY, my);
  if (blinds && t < W && !ginf[nt - 1]) {                        // window t of blind * h
    DigitIter it = load_scalar<FrP>(blinds, row, 1);
    uint32_t key = nb, neg = 0;
    for (int v = 0; v <= t; v++) it.next(v, C, W, nb, key, neg);
    if (key != nb) {
      Affine<F> a = Affine<F>::load(table + ((size_t)t * nt + nt - 1) * (Affine<F>::BYTES / 4));
      if (neg) a.y = a.y.neg();
      const B p = B::from_sat(XYZZ<F>::from_affine(a));
      const uint32_t d = key + 1;                                // 1 .. 2^(C-1)
      B acc = B::inf();
      for (int b = C - 1; b >= 0; b--) {
        acc = acc.dbl();
        if ((d >> b) & 1) acc.add(p);
      }
      acc.store(stg);
      B::add_mem(my, stg, my);
    }
  }
  __syncthreads();
  for (int h = PED_LANES / 2; h > 0; h >>= 1) {
    if (t < h) B::add_mem(my, my + (size_t)h * BY, my);
    __syncthreads();
  }
  if (t == 0) B::copy_point(rowsum + (size_t)row * BY, smem);
}

// launch 3 (and every level of key creation): n BkPoints -> canonical affine Montgomery points and identity flags
template <class F>
__global__ __launch_bounds__(PED_LANES) void ped_affine_kernel(const char* __restrict__ pts, uint32_t n, uint32_t* __restrict__ out_xy,
                                                               uint8_t* __restrict__ out_inf) {
  using B = BkPoint<F>;
  constexpr int FB = 4 * F::N;
  __shared__ __attribute__((aligned(16))) char tree[2 * PED_LANES * FB];     // node k at tree + k FB, leaves [PED_LANES, 2 PED_LANES)
  const int t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * PED_LANES + t;
  const bool act = i < n;
  const XYZZ<F> p = act ? B::load(pts + i * B::BYTES).to_sat() : XYZZ<F>::inf();
  const bool id = !act || p.is_inf();
  (id ? F::one() : p.zz * p.zzz).store(tree + (size_t)(PED_LANES + t) * FB);
  __syncthreads();
  for (int h = PED_LANES / 2; h >= 1; h >>= 1) {
    if (t < h) {
      const int k = h + t;
      (F::load(tree + (size_t)(2 * k) * FB) * F::load(tree + (size_t)(2 * k + 1) * FB)).store(tree + (size_t)k * FB);
    }
    __syncthreads();
  }
  if (t == 0) F::load(tree + FB).inv().store(tree + FB);
  __syncthreads();
  for (int h = 1; h < PED_LANES; h <<= 1) {                      // node k holds 1 / (its product): its children get theirs
    if (t < h) {
      const int k = h + t;
      const F ik = F::load(tree + (size_t)k * FB);
      const F a = F::load(tree + (size_t)(2 * k) * FB), b = F::load(tree + (size_t)(2 * k + 1) * FB);
      (ik * b).store(tree + (size_t)(2 * k) * FB);
      (ik * a).store(tree + (size_t)(2 * k + 1) * FB);
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
  const F e = F::load(tree + (size_t)(PED_LANES + t) * FB);      // 1 / (ZZ ZZZ)
  Affine<F>{p.x * (e * p.zzz), p.y * (e * p.zz)}.store(o);
  out_inf[i] = 0;
}

// key creation: generator i (flagged or (0, 0): the identity) -> cur[i]
template <class F>
__global__ __launch_bounds__(PED_LANES) void ped_key_load_kernel(const uint32_t* __restrict__ xy, const uint8_t* __restrict__ inf,
                                                                 uint32_t n, char* __restrict__ cur) {
  using B = BkPoint<F>;
  const size_t i = (size_t)blockIdx.x * PED_LANES + threadIdx.x;
  if (i >= n) return;
  const Affine<F> a = Affine<F>::load(xy + i * (2 * F::N));
  (inf[i] ? B::inf() : B::from_sat(XYZZ<F>::from_affine(a))).store(cur + i * B::BYTES);
}
// key creation: cur[i] <- 2^C cur[i]
template <class F, int C>
__global__ __launch_bounds__(PED_LANES) void ped_key_dbl_kernel(char* __restrict__ cur, uint32_t n) {
  using B = BkPoint<F>;
  const size_t i = (size_t)blockIdx.x * PED_LANES + threadIdx.x;
  if (i >= n) return;
  B p = B::load(cur + i * B::BYTES);
  for (int k = 0; k < C; k++) p = p.dbl();
  p.store(cur + i * B::BYTES);
}

// out (or the partial sums of chunk ch) [j] = sum over the chunk's rows of l[i] m[i cols + j]
template <class FrP>
__global__ __launch_bounds__(VECMAT_THREADS) void vecmat_kernel(const uint32_t* __restrict__ l, const uint32_t* __restrict__ m,
                                                                uint32_t rows, uint32_t cols, uint32_t col_blocks,
                                                                uint32_t* __restrict__ dst) {
  using F = Fp<FrP>;
  const uint32_t cb = blockIdx.x % col_blocks, ch = blockIdx.x / col_blocks;
  const uint32_t j = cb * VECMAT_THREADS + threadIdx.x;
  if (j >= cols) return;
  const uint32_t i0 = ch * VECMAT_ROW_CHUNK, i1 = min(rows, i0 + VECMAT_ROW_CHUNK);
  F acc = F::zero();
  for (uint32_t i = i0; i < i1; i++) acc = acc + F::load(l + (size_t)i * 8) * F::load(m + ((size_t)i * cols + j) * 8);
  acc.store(dst + ((size_t)ch * cols + j) * 8);
}
// out[j] = partial[0][j] + partial[1][j] + ... in this order
template <class FrP>
__global__ __launch_bounds__(VECMAT_THREADS) void vecmat_sum_kernel(const uint32_t* __restrict__ partial, uint32_t chunks, uint32_t cols,
                                                                    uint32_t* __restrict__ out) {
  using F = Fp<FrP>;
  const uint32_t j = blockIdx.x * VECMAT_THREADS + threadIdx.x;
  if (j >= cols) return;
  F acc = F::zero();
  for (uint32_t ch = 0; ch < chunks; ch++) acc = acc + F::load(partial + ((size_t)ch * cols + j) * 8);
  acc.store(out + (size_t)j * 8);
}

// ------------------------------------------------------------------------------------------- host
void key_create(zkp_ctx* ctx, const uint64_t* gens_xy_host, const uint8_t* gens_inf_host, size_t n_gens, const uint64_t* h_xy_host,
                zkp_pedersen_key** out) {
  using B = BkPoint<PdF>;
  constexpr size_t AB = Affine<PdF>::BYTES;
  ZKP_REQUIRE(n_gens >= 1 && n_gens <= PED_MAX_GENS, ZKP_ERR_BAD_ARG);
  const uint32_t nt = (uint32_t)n_gens + 1;
  // generators and h in one array; a (0, 0) point is flagged like a flagged one
  std::vector<uint8_t> xy(nt * AB), inf(nt, 0);
  memcpy(xy.data(), gens_xy_host, n_gens * AB);
  memcpy(xy.data() + n_gens * AB, h_xy_host, AB);
  for (uint32_t i = 0; i < nt; i++) {
    bool zero = true;
    for (size_t b = 0; b < AB && zero; b++) zero = xy[i * AB + b] == 0;
    inf[i] = zero || (i < n_gens && gens_inf_host && gens_inf_host[i]);
  }
  Scratch sc;
  const size_t o_xy = sc.take(nt * AB), o_inf = sc.take(nt), o_cur = sc.take((size_t)nt * B::BYTES), o_flags = sc.take(nt);
  sc.resolve(ctx->poly_tmp);
  hipStream_t st = ctx->cur->stream;
  zkp_pedersen_key* key = new zkp_pedersen_key;
  key->curve = PD_CURVE;
  key->ctx = ctx;
  key->n_gens = (uint32_t)n_gens;
  key->table_bytes = (size_t)PD_W * nt * AB;
  try {
    if (hipMalloc(reinterpret_cast<void**>(&key->table), key->table_bytes) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
    if (hipMalloc(reinterpret_cast<void**>(&key->inf), nt) != hipSuccess) throw StatusError{ZKP_ERR_OOM};
    ZKP_HIP(hipMemcpyAsync(sc.at<char>(o_xy), xy.data(), nt * AB, hipMemcpyHostToDevice, st));
    ZKP_HIP(hipMemcpyAsync(sc.at<char>(o_inf), inf.data(), nt, hipMemcpyHostToDevice, st));
    const unsigned blocks = (nt + PED_LANES - 1) / PED_LANES;
    hipLaunchKernelGGL(ped_key_load_kernel<PdF>, dim3(blocks), dim3(PED_LANES), 0, st, sc.at<uint32_t>(o_xy), sc.at<uint8_t>(o_inf), nt,
                       sc.at<char>(o_cur));
    for (int w = 0; w < PD_W; w++) {
      hipLaunchKernelGGL(ped_affine_kernel<PdF>, dim3(blocks), dim3(PED_LANES), 0, st, sc.at<char>(o_cur), nt,
                         key->table + (size_t)w * nt * (AB / 4), w == 0 ? key->inf : sc.at<uint8_t>(o_flags));
      if (w + 1 < PD_W)
        hipLaunchKernelGGL((ped_key_dbl_kernel<PdF, PD_C>), dim3(blocks), dim3(PED_LANES), 0, st, sc.at<char>(o_cur), nt);
    }
    ZKP_HIP(hipGetLastError());
    ZKP_HIP(hipStreamSynchronize(st));                             // the host arrays above are read until here
  } catch (...) {
    if (key->table) (void)hipFree(key->table);
    if (key->inf) (void)hipFree(key->inf);
    delete key;
    throw;
  }
  *out = key;
}

void commit_rows(zkp_ctx* ctx, const zkp_pedersen_key* key, const uint64_t* scalars_dev, size_t rows, size_t cols,
                 const uint64_t* blinds_dev, uint64_t* out_xy_dev, uint8_t* out_inf_dev) {
  using B = BkPoint<PdF>;
  constexpr size_t AB = Affine<PdF>::BYTES;
  ZKP_REQUIRE(key->ctx == ctx && key->curve == PD_CURVE, ZKP_ERR_BAD_ARG);
  ZKP_REQUIRE(rows >= 1 && cols >= 1 && cols <= key->n_gens && rows <= PED_MAX_CELLS / cols, ZKP_ERR_BAD_ARG);
  require_aligned16(scalars_dev);
  require_aligned16(blinds_dev);
  require_aligned16(out_xy_dev);
  require_disjoint_outputs({fr_span(scalars_dev, rows * cols, false), fr_span(blinds_dev, blinds_dev ? rows : 0, false),
                            MemSpan{(uintptr_t)out_xy_dev, (uintptr_t)out_xy_dev + rows * AB, true},
                            MemSpan{(uintptr_t)out_inf_dev, (uintptr_t)out_inf_dev + rows, true}});
  const PedersenPlan pl = pedersen_plan(ZKP_CFG_CURVE, (uint32_t)cols);
  ZKP_REQUIRE(pl.lds_bytes <= PED_LDS_MAX && pl.g * pl.W <= PED_MAX_ENTRIES, ZKP_ERR_DEVICE);   // cannot happen: the plan's own bounds
  Scratch sc;
  const size_t o_part = sc.take(rows * pl.S * B::BYTES), o_row = sc.take(rows * B::BYTES);
  sc.resolve(ctx->poly_tmp);
  hipStream_t st = ctx->cur->stream;
  const uint32_t nt = key->n_gens + 1;
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(scalars_dev);
  hipLaunchKernelGGL((ped_bucket_kernel<PdF, PdFr, PD_C, PD_W>), dim3((unsigned)(rows * pl.S)), dim3(PED_LANES), pl.lds_bytes, st,
                     key->table, key->inf, nt, sw, (uint32_t)cols, pl.S, pl.g, pl.G * pl.W, sc.at<char>(o_part));
  hipLaunchKernelGGL((ped_row_kernel<PdF, PdFr, PD_C, PD_W>), dim3((unsigned)rows), dim3(PED_LANES), 0, st, sc.at<char>(o_part), pl.S,
                     key->table, key->inf, nt, reinterpret_cast<const uint32_t*>(blinds_dev), sc.at<char>(o_row));
  hipLaunchKernelGGL(ped_affine_kernel<PdF>, dim3((unsigned)((rows + PED_LANES - 1) / PED_LANES)), dim3(PED_LANES), 0, st,
                     sc.at<char>(o_row), (uint32_t)rows, reinterpret_cast<uint32_t*>(out_xy_dev), out_inf_dev);
  ZKP_HIP(hipGetLastError());
}

void vecmat(zkp_ctx* ctx, const uint64_t* l_dev, const uint64_t* m_dev, size_t rows, size_t cols, uint64_t* out_dev) {
  ZKP_REQUIRE(rows >= 1 && cols >= 1 && rows <= PED_MAX_CELLS / cols, ZKP_ERR_BAD_ARG);
  require_aligned16(l_dev);
  require_aligned16(m_dev);
  require_aligned16(out_dev);
  require_disjoint_outputs({fr_span(l_dev, rows, false), fr_span(m_dev, rows * cols, false), fr_span(out_dev, cols, true)});
  const uint32_t chunks = (uint32_t)((rows + VECMAT_ROW_CHUNK - 1) / VECMAT_ROW_CHUNK);
  const uint32_t col_blocks = (uint32_t)((cols + VECMAT_THREADS - 1) / VECMAT_THREADS);
  hipStream_t st = ctx->cur->stream;
  uint32_t* out = reinterpret_cast<uint32_t*>(out_dev);
  uint32_t* dst = out;
  if (chunks > 1) {
    Scratch sc;
    const size_t o_part = sc.take((size_t)chunks * cols * 32);
    sc.resolve(ctx->poly_tmp);
    dst = sc.at<uint32_t>(o_part);
  }
  hipLaunchKernelGGL(vecmat_kernel<PdFr>, dim3(chunks * col_blocks), dim3(VECMAT_THREADS), 0, st, reinterpret_cast<const uint32_t*>(l_dev),
                     reinterpret_cast<const uint32_t*>(m_dev), (uint32_t)rows, (uint32_t)cols, col_blocks, dst);
  if (chunks > 1) hipLaunchKernelGGL(vecmat_sum_kernel<PdFr>, dim3(col_blocks), dim3(VECMAT_THREADS), 0, st, dst, chunks, (uint32_t)cols, out);
  ZKP_HIP(hipGetLastError());
}

const PedersenVtbl kVtbl = {key_create, commit_rows, vecmat};

}  // namespace pedersen_c<curve>

const PedersenVtbl* ZKP_PD_SYM(pedersen_vtbl_c, ZKP_CFG_CURVE)() { return &ZKP_PD_SYM(pedersen_c, ZKP_CFG_CURVE)::kVtbl; }

#if ZKP_CFG_CURVE == 0
// curve-independent pieces, once
const PedersenVtbl* pedersen_vtbl(int curve) {
  if (curve == ZKP_BN254) return pedersen_vtbl_c0();
  if (curve == ZKP_BLS12_381) return pedersen_vtbl_c1();
  throw StatusError{ZKP_ERR_UNSUPPORTED_CURVE};
}
void pedersen_key_free(zkp_ctx* ctx, zkp_pedersen_key* key) {
  ZKP_REQUIRE(key->ctx == ctx, ZKP_ERR_BAD_ARG);
  ZKP_HIP(hipStreamSynchronize(ctx->cur->stream));               // a commitment in flight still reads the tables
  (void)hipFree(key->table);
  (void)hipFree(key->inf);
  delete key;
}
void pedersen_key_info(const zkp_pedersen_key* key, uint64_t info[8]) {
  const PedersenPlan pl = pedersen_plan(key->curve == ZKP_BN254 ? 0 : 1, key->n_gens);
  info[0] = key->n_gens;
  info[1] = pl.c;
  info[2] = pl.W;
  info[3] = (uint64_t)pl.G * pl.W;
  info[4] = key->table_bytes;
  info[5] = pl.lds_bytes;
  info[6] = PED_LAUNCHES;
  info[7] = 0;
}
int pedersen_key_curve(const zkp_pedersen_key* key) { return key->curve; }
#endif

}  // namespace zkp
