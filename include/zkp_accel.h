/* zkp_accel.h — C ABI of the MI355X-native MSM + NTT proving backend for sec-bit/ckb-zkp.
 *
 * The reference (Rust) has no FFI for this path; this header *defines* the drop-in
 * boundary.  Each entry point names the reference call it replaces; INTEGRATION.md shows the Rust
 * `extern "C"` shim a maintainer would add.
 *
 * Conventions
 *   - every function returns int32_t: ZKP_OK (0) or a negative zkp_status; nothing throws across the ABI;
 *   - field elements: little-endian u64 limbs, MONTGOMERY form (R = 2^256, or 2^384 for BLS12-381 Fq)
 *     == ark-ff `Fp256/Fp384` in memory;  Fr = 4 limbs; Fq = 4 (BN254) / 6 (BLS12-381) limbs;
 *   - MSM scalars: 4 x u64 CANONICAL integers < r  == ark `BigInteger256` from `into_repr()`;
 *   - affine points: AoS (x, y), G2 coordinates (c0, c1); identity = separate u8 flag array (NULL = none);
 *   - projective results: ark Jacobian (X, Y, Z), identity = (0, 1, 0) — compare after `into_affine()`;
 *   - `*_dev` variants take DEVICE pointers (hipMalloc / torch tensors) and run on the ctx stream;
 *     host variants copy in/out and synchronise;
 *   - one in-flight call per ctx; create one ctx per prover thread / per GPU (one process per GPU): contexts on one device run
 *     concurrently from different host threads (the reference may prove from several rayon threads).  Since 0.5 every entry point
 *     that takes a ctx holds its lock for the whole call, so two threads entering the SAME ctx are serialised, never interleaved
 *     (0.6: zkp_set_profiling / zkp_*_last_timing too; the zkp_*_multi entry points hold the root's and every member's lock;
 *     zkp_ctx_destroy waits for a call in flight — destroying a context another thread still uses stays the caller's bug).
 */
#ifndef ZKP_ACCEL_H
#define ZKP_ACCEL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum { ZKP_BN254 = 0, ZKP_BLS12_381 = 1 } zkp_curve_t;

typedef enum {
  ZKP_OK = 0,
  ZKP_ERR_BAD_ARG = -1,
  ZKP_ERR_UNSUPPORTED_CURVE = -2,
  ZKP_ERR_DOMAIN_TOO_LARGE = -3, /* == SynthesisError::PolynomialDegreeTooLarge (groth16/src/r1cs_to_qap.rs:123-125) */
  ZKP_ERR_OOM = -4,
  ZKP_ERR_DEVICE = -5,           /* HIP runtime error, or no MI355X/gfx950 device: there is NO CPU fallback */
  ZKP_ERR_BAD_HANDLE = -6,
  ZKP_ERR_INVALID_POINT = -7 /* zkp_g*_decompress / zkp_g*_subgroup_check: a point is malformed / off the curve / outside the subgroup
                               (== ark-serialize SerializationError::InvalidData); *bad_index holds its index */
} zkp_status;

/* ops of zkp_ntt: ark-poly `EvaluationDomain::{fft,ifft,coset_fft,coset_ifft}_in_place`
 * (groth16/src/r1cs_to_qap.rs:144-148,161-162,169) */
typedef enum { ZKP_NTT_FFT = 0, ZKP_NTT_IFFT = 1, ZKP_NTT_COSET_FFT = 2, ZKP_NTT_COSET_IFFT = 3 } zkp_ntt_op;

typedef struct zkp_ctx zkp_ctx; /* opaque: device, stream, twiddle tables, scratch, resident bases */

const char* zkp_status_string(int32_t status);
/* "zkp_accel <major.minor> (gfx950)".  0.7.1: zkp_g1_ipa_fold_dev (IPA generator fold) / zkp_fr_dot_batch_dev (batched Fr inner
 * products); later in 0.7.1, detected by symbol: zkp_fr_sumcheck_round_dev (fused sum-check round) / zkp_fr_eq_evals_dev (eq
 * table), then zkp_fr_product_circuit_dev / zkp_fr_memcheck_circuits_dev (SPARK memory-checking hashes and product circuits),
 * then zkp_gkr_layer_upload / _free / _info and zkp_fr_gkr_eval_layer_dev / zkp_fr_gkr_tables_dev / zkp_fr_gkr_round_dev (Libra GKR),
 * then zkp_fr_prefix_product_dev / zkp_fr_plonk_perm_z_dev / zkp_fr_plonk_quotient_dev (PLONK rounds 2 and 3),
 * then zkp_fr_poly_eval_many_dev / zkp_fr_lincomb_dev (PLONK evaluations and opening polynomials),
 * then zkp_fr_gkr_eval_layer_batch_dev / zkp_fr_gkr_dp_round_dev (Hyrax data-parallel GKR),
 * then zkp_fr_powers_dev / zkp_fr_bp_t_coeffs_dev / zkp_fr_bp_lr_eval_dev / zkp_fr_ipa_fold_ab_dev (Bulletproofs R1CS prover),
 * then zkp_fr_asvc_subset_weights_dev / zkp_fr_asvc_quotient_dev (aSVC subvector commitments),
 * then zkp_pedersen_key_create / zkp_pedersen_key_free / zkp_pedersen_key_info / zkp_pedersen_commit_rows_dev / zkp_fr_vecmat_dev
 * (matrix polynomial commitments over a resident Pedersen key),
 * then zkp_g1_scale_vec_dev / zkp_g1_ntt_dev (per-lane scalar multiplication and the transform over G1 points),
 * then zkp_hash_params_create / zkp_hash_params_free / zkp_hash_params_info / zkp_fr_hash_blocks_dev / zkp_fr_hash_chain_dev /
 * zkp_fr_mimc_trace_dev / zkp_fr_merkle_tree_dev / zkp_fr_merkle_paths_dev (MiMC, Poseidon and Rescue hashing, CBMT Merkle trees),
 * then zkp_pairing_info / zkp_pairing_miller_dev / zkp_pairing_final_exp_dev / zkp_pairing_product_is_one_dev / zkp_pairing /
 * zkp_pairing_check (optimal-ate pairings: the Groth16 and KZG10 verifiers),
 * then zkp_sha256_info / zkp_sha256_dev / zkp_sha256_trace_dev / zkp_sha256_merkle_tree_dev / zkp_fr_bits_expand_dev (SHA-256
 * digests, traces and Merkle trees, and the witness of a bit circuit).
 * 0.7: zkp_msm_g1_var_batch_dev / zkp_msm_g2_var_batch_dev (batched small variable-base MSMs).
 * 0.6 (round 6): zkp_ctx_config / zkp_ctx_create_ex / zkp_ctx_create_multi_ex / zkp_ctx_get_config (the
 * prover switches are per context; the environment only supplies defaults, read when the context is created); RCCL bring-up behind a
 * watchdog (zkp_groth16_multi_info info[0] == 2); the multi-GPU entry points lock every member context.  0.5 (round 5): per-context lock (see Conventions); zkp_groth16_pk_upload_ex (ZKP_PK_KEEP_FORM); ZKP_MULTI_EXCHANGE=rccl also takes the RCCL
 * exchange with one rank; slots L / H of zkp_groth16_prove_partials_dev are only defined as a SUM for folded / evaluation-form /
 * bucket-chained keys (zkp_groth16_pk_info info[7] says which).  0.4 (round 4): ZKP_ERR_INVALID_POINT for malformed / out-of-subgroup points (0.2 used
 * ZKP_ERR_BAD_ARG), zkp_groth16_multi_info, zkp_bench_hbm_copy, zkp_groth16_points_into_affine; since 0.3 a bucket-chained key returns slot L of
 * zkp_groth16_prove_partials_dev as the identity and slot H as h + l (their sum is what prover.rs:189-196 consumes). */
const char* zkp_version(void);

/* ---- context & device memory ------------------------------------------------------------------ */
int32_t zkp_ctx_create(zkp_ctx** out, int device_id);
/* Per-context configuration (since 0.6; SURVEY §5 "Config / flags": struct, with the environment as the default).  A field left
 * at 0 means "default": the environment variable named beside it when the process has it set, else the built-in choice — so
 * zkp_ctx_create(out, dev) == zkp_ctx_create_ex(out, dev, NULL) and the A/B variables keep working.  A field that is set wins
 * over the environment and belongs to THIS context only: two contexts of one process may differ (the library keeps no other
 * prover state outside zkp_ctx).  Switches are tri-state: 0 default, ZKP_ON, ZKP_OFF. */
typedef enum { ZKP_DEFAULT = 0, ZKP_ON = 1, ZKP_OFF = 2 } zkp_tristate;
typedef enum { ZKP_EXCHANGE_AUTO = 0, ZKP_EXCHANGE_RCCL = 1, ZKP_EXCHANGE_PEER = 2 } zkp_exchange;
typedef struct {
  uint32_t struct_size;        /* sizeof(zkp_ctx_config) as the caller compiled it (fields beyond it are defaults); 0 is rejected */
  int32_t lanes;               /* proofs in flight inside zkp_groth16_prove_batch*: 1..8            [ZKP_LANES; 8, 4 above 2^22] */
  int32_t msm_batch_lanes;     /* lanes zkp_msm_g1_mont_batch_dev / Marlin's commitments rotate over [ZKP_BATCH_LANES; 1] */
  int32_t msm_window_bits;     /* bucket-index bits c of resident-table MSMs, 2..22                 [ZKP_MSM_C; round(log2 n) <= 20] */
  int32_t msm_window_bits_g2;  /* the same for G2 bases                                             [ZKP_MSM_C_G2; as G1] */
  int64_t msm_chunk_points;    /* lone G1 MSMs of >= 2x this many points run in chunks that share one bucket array; -1 = never
                                  chunk                                                             [ZKP_MSM_CHUNK; 3 * 2^19] */
  double table_budget_gb;      /* budget for resident window tables of this context, GiB            [ZKP_TABLE_BUDGET_GB; free
                                  device memory minus a quarter of the device] */
  int32_t h_evaluation_form;   /* tri-state: H query transformed to evaluation form at key upload   [ZKP_H_LAGRANGE; on] */
  int32_t c_fold;              /* tri-state: C matrix folded into the L query at key upload         [ZKP_C_FOLD; on] */
  int32_t host_affine;         /* tri-state: into_affine of the three proof points on the host      [ZKP_HOST_AFFINE; on] */
  int64_t c_fold_heavy_cost;   /* a C column above this cost (1 per +-1 coefficient, 380 per general one) leaves the fold kernel
                                  for one MSM of its own                                            [ZKP_LFOLD_HEAVY_COST; chosen per
                                  key: the cut that minimises longest kernel chain + 150 per heavy column, never below 1000] */
  int32_t multi_exchange;      /* ZKP_EXCHANGE_*: partial sums of zkp_groth16_prove_multi           [ZKP_MULTI_EXCHANGE; auto =
                                  RCCL all-gather when the devices are distinct and librccl loads, else peer copies] */
  int32_t multi_exchange_timeout_ms; /* watchdog of the RCCL setup and of the first all-gather: when it expires the key falls
                                  back to peer copies (said on stderr and in zkp_groth16_multi_info)  [ZKP_MULTI_EXCHANGE_TIMEOUT_MS; 30000] */
  int32_t multi_witness_split; /* tri-state: a / b / c chains of the witness map on devices 0 / 1 / 2 [ZKP_MULTI_WM_SPLIT;
                                  measured per key on proofs 3-4] */
} zkp_ctx_config;
/* cfg == NULL: all defaults.  ZKP_ERR_BAD_ARG for struct_size == 0 or a field out of range. */
int32_t zkp_ctx_create_ex(zkp_ctx** out, int device_id, const zkp_ctx_config* cfg);
/* the RESOLVED configuration of a context (defaults replaced by what the context actually uses; 0 where the choice depends on the
 * job, e.g. lanes / msm_window_bits) */
int32_t zkp_ctx_get_config(zkp_ctx* ctx, zkp_ctx_config* out);
int32_t zkp_ctx_destroy(zkp_ctx* ctx);
/* run on an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int32_t zkp_ctx_set_stream(zkp_ctx* ctx, void* hip_stream);
int32_t zkp_ctx_sync(zkp_ctx* ctx);
int32_t zkp_dev_alloc(zkp_ctx* ctx, size_t bytes, void** dptr);
int32_t zkp_dev_free(zkp_ctx* ctx, void* dptr);
int32_t zkp_h2d(zkp_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int32_t zkp_d2h(zkp_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* stream-ordered timing helpers (HIP events on the ctx stream) used by bench.py */
int32_t zkp_timer_start(zkp_ctx* ctx);
int32_t zkp_timer_stop_ms(zkp_ctx* ctx, float* ms);

/* ---- NTT: replaces ark-poly GeneralEvaluationDomain::<Fr> ops ----------------------------------
 * data: 2^log_n Fr elements (Montgomery), natural order in and out, in place.
 * log_n > 28 (BN254: its TWO_ADICITY) or > 30 (BLS12-381: TWO_ADICITY is 32, the library stops at 2^30) -> ZKP_ERR_DOMAIN_TOO_LARGE.
 * coset generator = Fr::multiplicative_generator() = 5 (BN254) / 7 (BLS12-381). */
int32_t zkp_ntt(zkp_ctx* ctx, zkp_curve_t curve, uint64_t* data_host, uint32_t log_n, int32_t op);
int32_t zkp_ntt_dev(zkp_ctx* ctx, zkp_curve_t curve, uint64_t* data_dev, uint32_t log_n, int32_t op);

/* ---- Fr vector / polynomial primitives around the Marlin prover's NTTs and KZG10 MSMs (device pointers) -----
 * vectors: Fr Montgomery, 4 x u64 per element.  k / z: one Fr element in HOST memory. */
typedef enum { ZKP_VEC_MUL = 0, ZKP_VEC_ADD = 1, ZKP_VEC_SUB = 2, ZKP_VEC_SCALE = 3, ZKP_VEC_AXPY = 4,
               ZKP_VEC_ADDC = 5 } zkp_vec_op;
/* out[i] = a[i]*b[i] | a[i]+b[i] | a[i]-b[i] | k*a[i] | a[i]+k*b[i] | a[i]+k   (marlin/src/ahp/prover.rs:248-252,298-305,399-411);
 * out may alias a or b */
int32_t zkp_fr_vec_op_dev(zkp_ctx* ctx, zkp_curve_t curve, int32_t op, const uint64_t* a, const uint64_t* b,
                          const uint64_t* k_host, uint64_t* out, size_t n);
/* sparse matrix-vector product, CSR on the device: out[i] = sum_k coeff[k] * x[col[k]]  (z_a = A z of
 * marlin/src/ahp/prover.rs:110-123; the `t` accumulation of :259-269 as a transposed product) */
int32_t zkp_fr_spmv_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint32_t* row_ptr_dev, const uint32_t* col_dev,
                        const uint64_t* coeff_dev, size_t nrows, const uint64_t* x_dev, uint64_t* out_dev);
/* out[i] = idx[i] < 0 ? 0 : in[idx[i]]   (interleaving of inputs/witness over H, prover.rs:176-186) */
int32_t zkp_fr_gather_dev(zkp_ctx* ctx, const uint64_t* in_dev, const int32_t* idx_dev, size_t n, uint64_t* out_dev);
/* DensePolynomial::divide_by_vanishing_poly (prover.rs:191,204,307,415): p = q (X^n - 1) + rem;
 * q_dev: len - n coefficients (or NULL), rem_dev: n coefficients (or NULL) */
int32_t zkp_poly_divide_by_vanishing_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* p_dev, size_t len, size_t n,
                                         uint64_t* q_dev, uint64_t* rem_dev);
/* stream-ordered device-to-device copy / zero fill (polynomial shifts, paddings) */
int32_t zkp_d2d(zkp_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
int32_t zkp_dev_zero(zkp_ctx* ctx, void* dst_dev, size_t bytes);
/* ark_ff::fields::batch_inversion, in place; zeros stay zero (marlin/src/ahp/prover.rs:357-367) */
int32_t zkp_fr_batch_inverse_dev(zkp_ctx* ctx, zkp_curve_t curve, uint64_t* v, size_t n);
/* DensePolynomial::evaluate (marlin/src/lib.rs:147-156): eval_out_host = sum_i p[i] z^i */
int32_t zkp_poly_evaluate_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* p, size_t n, const uint64_t* z_host,
                              uint64_t* eval_out_host);
/* KZG10 witness polynomial p / (X - z), remainder discarded (marlin/src/pc/kzg10.rs:211-226):
 * q_dev receives n-1 coefficients (q_dev != p); eval_out_host (optional) receives p(z) */
int32_t zkp_poly_div_linear_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* p, size_t n, const uint64_t* z_host,
                                uint64_t* q_dev, uint64_t* eval_out_host);

/* ---- bases (proving-key queries / SRS powers): upload once, prove many -------------------------
 * xy: n affine points (Montgomery); inf: n flags or NULL.  The library copies (and pre-computes its
 * window tables in HBM); the caller keeps ownership of the host buffers. */
int32_t zkp_bases_upload_g1(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n,
                            uint64_t* handle);
int32_t zkp_bases_upload_g2(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n,
                            uint64_t* handle);
int32_t zkp_bases_free(zkp_ctx* ctx, uint64_t handle);
/* Make a resident base vector of `src` usable through `dst` as well (same device, same process): the window tables are
 * shared, not copied — one SRS / proving key serves several contexts (one per prover thread).  The entry lives until
 * every context that holds it has freed it. */
int32_t zkp_bases_share(zkp_ctx* dst, zkp_ctx* src, uint64_t src_handle, uint64_t* dst_handle);
int32_t zkp_bases_len(zkp_ctx* ctx, uint64_t handle, size_t* n);

/* ---- MSM: replaces ark_ec::msm::VariableBaseMSM::multi_scalar_mul ------------------------------
 * (groth16/src/prover.rs:187,190,220; marlin/src/pc/kzg10.rs:109,118,137,146; curve/src/lib.rs:44)
 * result = sum_{i<n} scalars[i] * bases[offset+i]; n is clamped to the bases available (ark's
 * min(len) truncation, prover.rs:186-187); n == 0 -> identity.
 * out_xyz: 3 (G1) or 6 (G2) field elements, Jacobian, Montgomery, host memory. */
int32_t zkp_msm_g1(zkp_ctx* ctx, uint64_t handle, size_t offset, const uint64_t* scalars_host, size_t n,
                   uint64_t* out_xyz);
int32_t zkp_msm_g2(zkp_ctx* ctx, uint64_t handle, size_t offset, const uint64_t* scalars_host, size_t n,
                   uint64_t* out_xyz);
int32_t zkp_msm_g1_dev(zkp_ctx* ctx, uint64_t handle, size_t offset, const uint64_t* scalars_dev, size_t n,
                       uint64_t* out_xyz_host);
int32_t zkp_msm_g2_dev(zkp_ctx* ctx, uint64_t handle, size_t offset, const uint64_t* scalars_dev, size_t n,
                       uint64_t* out_xyz_host);
/* zkp_curve::Curve::vartime_multiscalar_mul (curve/src/lib.rs:38-45): scalars are Fr in MONTGOMERY form;
 * the into_repr() map is fused into the digit scan on the device. */
int32_t zkp_vartime_multiscalar_mul_g1(zkp_ctx* ctx, uint64_t handle, const uint64_t* fr_scalars_host, size_t n,
                                       uint64_t* out_xyz);
int32_t zkp_vartime_multiscalar_mul_g2(zkp_ctx* ctx, uint64_t handle, const uint64_t* fr_scalars_host, size_t n,
                                       uint64_t* out_xyz);
/* TRUE variable-base MSM — the literal semantics of `VariableBaseMSM::multi_scalar_mul(bases, scalars)` and of
 * `Curve::vartime_multiscalar_mul(scalars, points)` (curve/src/lib.rs:38-45) when the bases are FRESH on every call
 * (bulletproofs / spartan / hyrax generators): points and scalars come from HOST memory, nothing is precomputed and
 * nothing stays resident (no window tables: W = 256 / c separate bucket sets, c = 16 from 2^12 points on, and a
 * <= 255-doubling tail).  montgomery != 0: scalars are Fr elements (into_repr() fused), else canonical BigInteger256.
 * Use the resident-handle entry points above when the same bases serve many MSMs (proving keys, SRS): they are ~3x faster. */
int32_t zkp_msm_g1_var(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy_host, const uint8_t* inf_host,
                       const uint64_t* scalars_host, size_t n, int32_t montgomery, uint64_t* out_xyz);
int32_t zkp_msm_g2_var(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy_host, const uint8_t* inf_host,
                       const uint64_t* scalars_host, size_t n, int32_t montgomery, uint64_t* out_xyz);
/* `count` independent TRUE variable-base MSMs (curve/src/lib.rs:38-45 with fresh bases; hyrax IPA rounds, bulletproofs) in one
 * call: result k = sum_{i < ns[k]} scalars_dev[k][i] * bases xy_dev[k][i].  Points, flags and scalars are in DEVICE memory (xy_dev[k]
 * and scalars_dev[k] 16-byte aligned, as any element of a zkp_dev_alloc buffer is); nothing is precomputed or kept resident.
 * inf_dev == NULL or inf_dev[k] == NULL: no identity flags for that entry.  montgomery != 0: Fr in Montgomery form (into_repr()
 * fused), else canonical BigInteger256.  ns[k] == 0 -> identity.  Entries may alias (same bases or scalars for many k).
 * Two kernel launches per call whatever `count` is: one wave per (entry, window, slice of <= 4096 points) with its 2^(c-1) XYZZ
 * buckets in LDS (c = 8, or 9 from 2^13 points on), then one wave per entry for the window weights.  The caps bound the
 * ~255-doubling tail and the slice partials per entry; above them the sort-based pipeline of zkp_msm_g*_var (c = 16, shared
 * bucket reduction) does less work per point.  G2 points are twice as costly per addition, so its cap is half.
 * ns[k] > cap -> ZKP_ERR_BAD_ARG (use zkp_msm_g*_var above that).  Every argument is checked before anything runs: on an error
 * out_xyz is untouched.  Runs on the context's current stream and returns after the results are on the host.
 * out_xyz: count Jacobian Montgomery results, 3 (G1) / 6 (G2) field elements each, host memory. */
#define ZKP_MSM_SMALL_MAX_G1 65536
#define ZKP_MSM_SMALL_MAX_G2 32768
int32_t zkp_msm_g1_var_batch_dev(zkp_ctx* ctx, zkp_curve_t curve, size_t count, const uint64_t* const* xy_dev,
                                 const uint8_t* const* inf_dev, const uint64_t* const* scalars_dev, const size_t* ns,
                                 int32_t montgomery, uint64_t* out_xyz);
int32_t zkp_msm_g2_var_batch_dev(zkp_ctx* ctx, zkp_curve_t curve, size_t count, const uint64_t* const* xy_dev,
                                 const uint8_t* const* inf_dev, const uint64_t* const* scalars_dev, const size_t* ns,
                                 int32_t montgomery, uint64_t* out_xyz);
/* IPA generator fold (spartan/src/inner_product.rs:71-74, hyrax/src/commitment.rs:550-552):
 * out[i] = (a * L[i] + b * R[i]).into_affine() for i < n, BN254 / BLS12-381 G1.
 * l_xy, r_xy, out_xy: n affine Montgomery points in DEVICE memory, the layout of zkp_bases_upload_g1 / zkp_msm_g1_var_batch_dev
 * (16-byte aligned).  l_inf / r_inf: identity flags or NULL (= none).  out_inf: required.
 * a_host, b_host: one Fr element each, Montgomery, host memory.  The same a and b apply to every i.
 * Identities are written exactly as zkp_fixed_base_mul_g1 writes them (words and flag).
 * out_xy may equal l_xy or r_xy, and out_inf may equal l_inf or r_inf (in-place fold).  Any other overlap -> ZKP_ERR_BAD_ARG.
 * n == 0 -> ZKP_OK, nothing runs.  Every argument is checked before anything runs: on an error the outputs are untouched.
 * One launch: one lane per point, GLV + joint-sparse-form digits of a and b planned once on the host, one batch inversion per
 * 64 points.  Runs on the context's current stream and returns when out is written. */
int32_t zkp_g1_ipa_fold_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* l_xy, const uint8_t* l_inf,
                            const uint64_t* r_xy, const uint8_t* r_inf, size_t n,
                            const uint64_t* a_host, const uint64_t* b_host, uint64_t* out_xy, uint8_t* out_inf);
/* count inner products <a_k, b_k> of Fr Montgomery vectors in DEVICE memory (16-byte aligned), ns[k] terms each (0 -> zero);
 * entries may alias.  out_host: count Fr elements, Montgomery.  Two launches whatever count is (spartan/src/inner_product.rs:40-41).
 * Every argument is checked before anything runs.  Returns after the results are on the host. */
int32_t zkp_fr_dot_batch_dev(zkp_ctx* ctx, zkp_curve_t curve, size_t count, const uint64_t* const* a_dev,
                             const uint64_t* const* b_dev, const size_t* ns, uint64_t* out_host);
/* One sum-check round over dense multilinear tables of Fr (spartan/src/prover.rs:422-592, 594-723, 1442-1607): bind the previous
 * challenge into every table (combine_with_r, polynomial.rs:130-138) and evaluate the next round polynomial of `count` terms at
 * t = 0, 2, (3) (combine_with_n, polynomial.rs:121-128) in ONE pass over the tables plus one small launch that adds the
 * per-workgroup partial sums.  g(1) is not computed: it is claim - g(0).
 *   kind                    g                 tables per term (in this order)   points returned
 *   ZKP_SC_EQ_AB_MINUS_C    eq (a b - c)      eq, a, b, c                       g(0), g(2), g(3)
 *   ZKP_SC_PROD2            a b               a, b                              g(0), g(2)
 *   ZKP_SC_PROD3            a b c             a, b, c                           g(0), g(2), g(3)
 * tables_dev: count * arity(kind) device pointers (host array), each to len Fr (Montgomery, 16-byte aligned), len a power of two.
 * bind_host != NULL: every DISTINCT table becomes combine_with_r(table, *bind_host) in place over [0, len/2), i.e.
 *   t[j] = t[j] + x (t[j + len/2] - t[j]); elements [len/2, len) are left untouched; then len /= 2.
 * evals_out_host != NULL: count * npoints(kind) Fr (Montgomery), term-major, of the (bound) tables:
 *   g(t) = sum_{j < len/2} g(lo_j + t (hi_j - lo_j)) with lo_j = t[j], hi_j = t[j + len/2] per table.
 * The same pointer may appear in several terms, or several times in one term: it is bound exactly once.
 * ZKP_ERR_BAD_ARG: NULL or misaligned tables, len not a power of two or > 2^28, len < 2 with bind_host, a length below 2 at
 * evaluation time, both bind_host and evals_out_host NULL, an unknown kind, *bind_host >= r, count > 256, two tables that overlap
 * without being the same pointer.  Every argument is checked before anything runs: on an error nothing is written.
 * Scratch: count * npoints(kind) * len / 16 bytes of partial sums (len / 32 with bind_host) from the context's grow-only arena;
 * ZKP_ERR_OOM (nothing written) if the device cannot hold them, which only many terms over tables near 2^28 rows can reach.
 * count == 0 -> ZKP_OK.  Runs on the context's current stream and returns after the evaluations are on the host.
 * A proof of v rounds is v + 1 calls: (NULL, evals), then (r_{i-1}, evals) ..., then (r_{v-1}, NULL), which leaves the final
 * values at element 0 of each table. */
typedef enum { ZKP_SC_EQ_AB_MINUS_C = 0, ZKP_SC_PROD2 = 1, ZKP_SC_PROD3 = 2 } zkp_sumcheck_kind;
int32_t zkp_fr_sumcheck_round_dev(zkp_ctx* ctx, zkp_curve_t curve, int32_t kind, size_t count, uint64_t* const* tables_dev,
                                  size_t len, const uint64_t* bind_host, uint64_t* evals_out_host);
/* eval_eq (spartan/src/polynomial.rs:8-24): out_dev[idx] = prod_i (bit_{k-1-i}(idx) ? r[i] : 1 - r[i]) for idx < 2^k, so r[0]
 * decides the most significant bit of the index; k == 0 -> [1].  r_host: k Fr (Montgomery, each < r), host memory; out_dev: 2^k Fr
 * (Montgomery, 16-byte aligned), device memory.  k > 28 or an r_host[i] >= r -> ZKP_ERR_BAD_ARG.  One launch. */
int32_t zkp_fr_eq_evals_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* r_host, size_t k, uint64_t* out_dev);
/* SPARK memory checking (later in 0.7.1, detected by symbol): the product circuits of `memory_checking` that
 * product_circuit_eval_prover walks (spartan/src/spark.rs:209-347, prover.rs:1313-1440), every layer kept on the device.
 *
 * construct_product_circuit (spark.rs:315-347) for `count` circuits of n leaves each, layer 0 already in place.
 * circuits_dev: count device pointers (host array); circuits_dev[k]: 2n - 2 Fr (Montgomery, canonical, 16-byte aligned).
 * Layer l (n >> l elements, l = 0 .. log2 n - 1) starts at element 2n - (2n >> l); left_vec[l] / right_vec[l] of the reference are
 * the first / second half of layer l:  layer[l+1][j] = layer[l][j] * layer[l][j + (n >> (l+1))].
 * roots_host[k] (count Fr, Montgomery, host memory) = evaluate_product_circuit (spark.rs:349-359) = last layer's [0] * [1].
 * n: a power of two, 2 <= n <= 2^28 (the reference's padding of odd lengths with 1 is never reached by Spartan's power-of-two tables
 * and is not built); 1 <= count <= 256.  ZKP_ERR_BAD_ARG, before anything is launched or written: a NULL context or array, a NULL or
 * misaligned circuits_dev[k], an n or count outside these rules, circuit buffers that overlap each other.
 * Every element written is the canonical Montgomery representative (bit-exact results).  ceil((log2 n - 9) / 3) + 1 launches for
 * n > 512, one below, whatever count is.  Runs on the context's current stream and returns after the roots are on the host. */
int32_t zkp_fr_product_circuit_dev(zkp_ctx* ctx, zkp_curve_t curve, size_t count, uint64_t* const* circuits_dev, size_t n,
                                   uint64_t* roots_host);
/* circuit_hash minus gamma2 (spark.rs:223-273, 298-312) written as layer 0 of circuit k, then the circuit as above:
 *   leaf[i] = addr[i] * gamma1^2 + val[i] * gamma1 + (ts[i] + ts_add[k]) - gamma2
 * addr_dev[k] == NULL: addr[i] = i (init / audit).  ts_dev[k] == NULL: ts[i] = 0 (init).  ts_add[k] is 0 or 1 (write = read + 1).
 * addr_dev / val_dev / ts_dev / circuits_dev: host arrays of count device pointers; ts_add: count values, host memory.
 * addr and ts are n uint32 each on the device, val is n Fr (Montgomery, 16-byte aligned).  gamma1_host / gamma2_host: one Fr each
 * (Montgomery, < r), host memory.  Inputs may be shared between entries (the read and write circuits of a list share addr, val and
 * ts: such a pair is hashed once); circuit buffers must not overlap each other or the inputs.
 * ZKP_ERR_BAD_ARG, before anything is launched or written: the rules of zkp_fr_product_circuit_dev, a NULL or misaligned val_dev[k],
 * a misaligned addr_dev[k] / ts_dev[k], ts_add[k] > 1, a gamma >= r, a circuit buffer that overlaps an input.
 * The leaf pass is fused into the first launch: the launch count is that of zkp_fr_product_circuit_dev. */
int32_t zkp_fr_memcheck_circuits_dev(zkp_ctx* ctx, zkp_curve_t curve, size_t count, const uint32_t* const* addr_dev,
                                     const uint64_t* const* val_dev, const uint32_t* const* ts_dev, const uint32_t* ts_add,
                                     uint64_t* const* circuits_dev, size_t n, const uint64_t* gamma1_host,
                                     const uint64_t* gamma2_host, uint64_t* roots_host);
/* Libra's linear-time GKR (later in 0.7.1, detected by symbol): the table work of one circuit layer in the loop of
 * LinearGKRProof::prover (libra/src/libra_linear_gkr.rs:22-114) and of its ZK twin (libra_zk_linear_gkr.rs), every table kept on
 * the device.  Commitments, blinds and the transcript stay with the caller.
 *
 * The wiring of one layer, Layer::mid_layer_new (libra/src/circuit.rs:55-80): gate g = (op[g], left[g], right[g]), op 0 = add,
 * 1 = mul, left / right < 2^log_in the nodes of the layer below.  op_host / left_host / right_host: n_gates values each, host
 * memory.  1 <= n_gates <= 2^28, log_in <= 28; log_out = ceil(log2 n_gates).  ZKP_ERR_BAD_ARG, before anything is allocated: a
 * NULL context or array, any other op (IllegalOperator), a node >= 2^log_in (IllegalNode), n_gates or log_in outside these rules.
 * The host sorts the gates once (counting sort): natural order, grouped by left node and grouped by right node (gate order
 * within a node's segment), and cuts every segment of more than 256 entries into chunks of 4096 (the long segments); then it
 * uploads them.  About 24 n_gates + 8 * 2^log_in bytes of device memory.  The handle belongs to the context's device. */
typedef struct zkp_gkr_layer zkp_gkr_layer;
int32_t zkp_gkr_layer_upload(zkp_ctx* ctx, const uint8_t* op_host, const uint32_t* left_host, const uint32_t* right_host,
                             size_t n_gates, uint32_t log_in, zkp_gkr_layer** layer);
int32_t zkp_gkr_layer_free(zkp_ctx* ctx, zkp_gkr_layer* layer);
/* info: n_gates, log_out, log_in, mul gates, largest fan-out by left node, by right node, long segments by left node, by right node */
int32_t zkp_gkr_layer_info(const zkp_gkr_layer* layer, uint64_t info[8]);
/* One layer of Circuit::evaluate (circuit.rs:140-185; hyrax/src/circuit.rs has the same gate model) with the padding of eval_output
 * (evaluate.rs:16-21):  out[g] = op[g] ? in[left[g]] * in[right[g]] : in[left[g]] + in[right[g]]  for g < n_gates, out[g] = 0 for
 * n_gates <= g < 2^log_out.  in_dev: 2^log_in Fr, out_dev: 2^log_out Fr (Montgomery, canonical, 16-byte aligned, device memory);
 * they must not overlap.  One launch.  Returns when out_dev is written. */
int32_t zkp_fr_gkr_eval_layer_dev(zkp_ctx* ctx, zkp_curve_t curve, const zkp_gkr_layer* layer, const uint64_t* in_dev,
                                  uint64_t* out_dev);
/* The bookkeeping tables of one phase from ONE pass over the gates.  g_dev: 2^log_out Fr (G = alpha eq(gu) + beta eq(gv)),
 * w_dev: 2^log_in Fr, out_dev: host array of 3 device pointers to 2^log_in Fr each.  With x = left[g], y = right[g]:
 *   phase 1, eval_hg (evaluate.rs:79-99), w = V:        mul gates: out[0][x] += G[g] w[y]
 *                                                       add gates: out[1][x] += G[g], out[2][x] += G[g] w[y]
 *   phase 2, eval_fgu (evaluate.rs:101-119), w = eq(ru): mul gates: out[0][y] += G[g] w[x]
 *                                                       add gates: out[1][y] += G[g] w[x];  out_dev[2] must be NULL
 * Every slot of every output is written; a node without gates gets 0.  One field product per gate, no atomics: the thread that
 * owns a node adds its segment; a long segment is added by one workgroup per chunk, then one workgroup per segment.  One launch
 * when the layer has no long segment on that side (info[6] / info[7] == 0), three otherwise.
 * ZKP_ERR_BAD_ARG, before anything is launched or written: a NULL or misaligned pointer, a phase other than 1 or 2, out_dev[2] != NULL
 * in phase 2, an output that overlaps another output or an input.  ZKP_ERR_BAD_HANDLE: a layer of another device.
 * Every element written is the canonical Montgomery representative (bit-exact results). */
int32_t zkp_fr_gkr_tables_dev(zkp_ctx* ctx, zkp_curve_t curve, const zkp_gkr_layer* layer, int32_t phase, const uint64_t* g_dev,
                              const uint64_t* w_dev, uint64_t* const* out_dev);
/* One round of phase_one_prover / phase_two_prover (libra/src/sumcheck.rs:21-97, 99-173; the ZK variants :186-426 run the same
 * table work): bind the previous challenge into every table (combine_with_r, evaluate.rs:43-51) and evaluate the next round
 * polynomial at t = 0 and t = 2 in ONE pass, plus one small launch that adds the per-workgroup partial sums.
 *   phase 1: tables_dev = f, mul, add1, add2;  g = f (mul + add1) + add2;  fu_host is not read
 *   phase 2: tables_dev = f, mul, add;         g = fu (mul f + add) + add f;  fu_host: one Fr (Montgomery, < r), host memory
 * tables_dev: host array of 4 / 3 distinct device pointers, each to len Fr (Montgomery, 16-byte aligned), len a power of two.
 * bind_host, the untouched elements [len/2, len), evals_out_host == NULL (bind only) and bind_host == NULL (round 0) are those of
 * zkp_fr_sumcheck_round_dev; evals_out_host: 2 Fr (Montgomery), g(0) then g(2); g(1) is claim - g(0).
 * ZKP_ERR_BAD_ARG, before anything runs: a phase other than 1 or 2, NULL or misaligned tables, tables that overlap, len not a power
 * of two or > 2^28, len < 2 with bind_host, a length below 2 at evaluation time, both bind_host and evals_out_host NULL,
 * *bind_host >= r, in phase 2 *fu_host >= r or a NULL fu_host with evals_out_host.
 * Two launches for a call that evaluates, one for a bind-only call.  Returns after the evaluations are on the host. */
int32_t zkp_fr_gkr_round_dev(zkp_ctx* ctx, zkp_curve_t curve, int32_t phase, uint64_t* const* tables_dev, size_t len,
                             const uint64_t* fu_host, const uint64_t* bind_host, uint64_t* evals_out_host);
/* Hyrax's data-parallel GKR (later in 0.7.1, detected by symbol): n copies of one layered circuit proved at once, the table work of
 * one layer in the loop of HyraxProof::prover (hyrax/src/hyrax_proof.rs:92-147).  The wiring is a zkp_gkr_layer (hyrax/src/circuit.rs
 * has Libra's gate model).  Pedersen and packing commitments, blinds and the transcript stay with the caller.
 * A layer's values over all copies are NODE-MAJOR: V[i n + t] is node i in copy t, i < 2^log_in, n a power of two,
 * log_in + log2 n <= 28; Fr, Montgomery, canonical, 16-byte aligned, device memory.
 *
 * One layer of Circuit::evaluate (hyrax/src/circuit.rs:115-163) over n copies, with the zero rows of hyrax_proof.rs:104-107:
 *   out[g n + t] = op[g] ? in[left[g] n + t] * in[right[g] n + t] : in[left[g] n + t] + in[right[g] n + t]   for g < n_gates,
 *   out[g n + t] = 0 for n_gates <= g < 2^log_out.   in_dev: 2^log_in n Fr, out_dev: 2^log_out n Fr (log_out + log2 n <= 28 too);
 * they must not overlap.  One launch.  ZKP_ERR_BAD_ARG, before anything runs: a NULL or misaligned pointer, n not a power of two,
 * a size above these limits, out_dev over in_dev.  ZKP_ERR_BAD_HANDLE: a layer of another device.  Returns when out_dev is written. */
int32_t zkp_fr_gkr_eval_layer_batch_dev(zkp_ctx* ctx, zkp_curve_t curve, const zkp_gkr_layer* layer, const uint64_t* in_dev,
                                        uint64_t* out_dev, size_t n);
/* One round of sum-check #1 of ZkSumcheckProof::prover (hyrax/src/zk_sumcheck_proof.rs:98-220), the one over the copy variables.
 * The reference keeps one table of n elements per gate (temp_vec, :83-95); it is rank one, temp_vec[g][t] = w[g] eq[t] with
 * w[g] = u0 eq(ql)[g] + u1 eq(qr)[g] and eq = eq(q'), and combine_with_r (hyrax/src/evaluate.rs:101-109) keeps it so: the call takes
 * the n-element eq table and the weight vector instead.
 *   v_dev:  2^log_in rows of stride n, the layer below over all copies (circuit_evals, hyrax_proof.rs:95-107); len live per row
 *   eq_dev: n Fr, len live;   w_dev: 2^log_out Fr, of which the first n_gates are read;   len <= n, both powers of two
 * bind_host != NULL (one Fr, Montgomery, < r, host memory): first every one of the 2^log_in rows, referenced by a gate or not, and
 * eq become t[j] + x (t[j + len/2] - t[j]) over [0, len/2), in place (:191-203); [len/2, len) is untouched; then len /= 2.
 * evals_out_host != NULL: three Fr (Montgomery), g(0), g(2), g(3) of
 *   g(X) = sum_{j < len/2} eq_X[j] sum_g w[g] op_g(L_X[j], R_X[j]),   every table at lo + X (hi - lo)   (:103-156);
 * g(1) is claim - g(0).  finals_dev != NULL (2^log_in Fr, device memory): allowed only when the length after the bind is 1;
 * finals[i] = V[i n], the v_vec of :222-224.  A proof of v rounds is v + 1 calls, as for zkp_fr_sumcheck_round_dev: round 0
 * without bind_host, the closing call without evals_out_host.
 * ZKP_ERR_BAD_ARG, before anything runs or is written: a NULL v_dev / eq_dev / w_dev, a misaligned pointer, n or len not a power of
 * two, len > n, log_in + log2 n > 28, len < 2 with bind_host, a length below 2 at evaluation time, both bind_host and
 * evals_out_host NULL, *bind_host >= r, finals_dev with a resulting length other than 1, v / eq / finals overlapping each other
 * or w, more than 2^20 workgroups (ceil(columns / 256) * ceil(n_gates / 32), columns = half the length at evaluation time).
 * ZKP_ERR_BAD_HANDLE: a layer of another device.
 * The evaluation walks the gates grouped by their left node in chunks of 32 entries, one workgroup per 256 columns and chunk:
 * two field products per gate and three more per node that has a mul gate, no atomics, no hand-off between workgroups.  Three launches for a call
 * that binds and evaluates, two for round 0, one for the closing call.  Bit-exact results.  Returns after the evaluations are on
 * the host. */
int32_t zkp_fr_gkr_dp_round_dev(zkp_ctx* ctx, zkp_curve_t curve, const zkp_gkr_layer* layer, uint64_t* v_dev, uint64_t* eq_dev,
                                const uint64_t* w_dev, size_t n, size_t len, const uint64_t* bind_host, uint64_t* evals_out_host,
                                uint64_t* finals_dev);
/* The Bulletproofs R1CS prover (later in 0.7.1, detected by symbol): the Fr work of `prove` (bulletproofs/src/arithmetic_circuit.rs:
 * 305-612) and of inner_product_proof::prove (inner_product_proof.rs:22-111), every vector kept on the device.  The commitments are
 * zkp_msm_g1_var_batch_dev calls, the generator folds zkp_g1_ipa_fold_dev; the transcript stays with the caller.  Vectors: Fr,
 * Montgomery, canonical, 16-byte aligned, device memory.  Scalars (*_host): Fr, Montgomery, < r, host memory.  Every element written is
 * the canonical Montgomery representative (bit-exact results).  Every argument is checked before anything runs: on ZKP_ERR_BAD_ARG
 * every output is untouched.  Each call runs on the context's current stream and returns when its outputs are written.
 * A pass runs T = 256 * min(ceil(n / 256), 512) threads; thread j owns the indices j, j + T, ..., forms its powers once (one product
 * per set bit of j, from the squarings base^(2^b) that the host passes) and steps by their T-th powers (computed on the host), the
 * ownership of zkp_fr_poly_eval_many_dev.
 *
 * out[i] = first * ratio^i for i < n (y_n, z_Q of :411-433; z_Q is the vector zkp_fr_spmv_dev multiplies into the transposed
 * constraint matrices).  One launch.  n == 0 -> ZKP_OK, nothing runs.  ratio == 0 gives [first, 0, ...].
 * ZKP_ERR_BAD_ARG: a NULL or misaligned out_dev, n > 2^28, *first_host or *ratio_host >= r. */
int32_t zkp_fr_powers_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* first_host, const uint64_t* ratio_host, uint64_t* out_dev,
                          size_t n);
/* The inputs of l(X) and r(X): the padded vectors of :399-409 without their padding.  An index at or beyond a vector's length counts
 * as zero and is never dereferenced; a pointer whose length is 0 may be NULL.  N: a power of two, at least each length, <= 2^28.
 * v is the caller's zQ * WV (:469), n_w elements. */
typedef struct {
  const uint64_t* aL; /* n elements */
  const uint64_t* aR; /* n */
  const uint64_t* aO; /* n */
  const uint64_t* w;  /* n_w: the witness */
  const uint64_t* v;  /* n_w */
  const uint64_t* sL; /* n_s: the blinding vectors */
  const uint64_t* sR; /* n_s */
  size_t n;
  size_t n_w;
  size_t n_s;
  size_t N;
} zkp_bp_vectors;
/* The coefficients t2 .. t10 of t(X) = <l(X), r(X)> (VecPoly5::special_inner_product, bulletproofs/src/lib.rs:223-250), t4 included:
 * t_out_host receives 9 Fr.  With the diagonal WL, WR, WO of :436-445 written out, for i < N:
 *   Y_i = y^i,  Z_i = z^(i+1) for i < n else 0,  zn = z^n,  U_i = zn Z_i y^(-i)
 *   l2 = aL + U,  l3 = aO,  l4 = w,  l5 = sL;    r0 = -v,  r1 = zn^2 Z - Y,  r2 = Y aR + Z,  r5 = Y sR      (:471-489)
 * No coefficient vector is stored: one pass over the seven inputs forms them in registers (U as one progression of ratio z / y, y
 * inverted once on the host) and leaves nine partial sums per workgroup, reduced three at a time through one LDS buffer; one small
 * launch adds them.  Two launches.  ZKP_ERR_BAD_ARG: a NULL vecs, N not a power of two or > 2^28, a length above N, a NULL or
 * misaligned vector of nonzero length, *y_host == 0, *y_host or *z_host >= r. */
int32_t zkp_fr_bp_t_coeffs_dev(zkp_ctx* ctx, zkp_curve_t curve, const zkp_bp_vectors* vecs, const uint64_t* y_host,
                               const uint64_t* z_host, uint64_t* t_out_host);
/* l(x) and r(x) (VecPoly5::eval, :528-529) from the same coefficients, formed again in registers, and t_x = <l(x), r(x)> (:531):
 *   l_x[i] = x^2 (l2 + x (l3 + x (l4 + x l5))),   r_x[i] = r0 + x r1 + x^2 r2 + x^5 r5   for i < N;   *t_x_out_host = sum_i l_x[i] r_x[i].
 * l_x_dev, r_x_dev: N Fr each; they overlap neither each other nor any input.  Two launches.
 * ZKP_ERR_BAD_ARG: the rules of zkp_fr_bp_t_coeffs_dev, *x_host >= r, a NULL or misaligned output, an output that overlaps the
 * other output or an input. */
int32_t zkp_fr_bp_lr_eval_dev(zkp_ctx* ctx, zkp_curve_t curve, const zkp_bp_vectors* vecs, const uint64_t* y_host,
                              const uint64_t* z_host, const uint64_t* x_host, uint64_t* l_x_dev, uint64_t* r_x_dev,
                              uint64_t* t_x_out_host);
/* The a / b half of one round of inner_product_proof::prove (:93-95) together with the NEXT round's inner products (:54-55).
 * n: a power of two, 2 <= n <= 2^28; m = n / 2.  In place over the low halves, the high halves [m, n) are left untouched:
 *   a[j] = x a[j] + x^-1 a[j + m],   b[j] = x^-1 b[j] + x b[j + m]   for j < m.
 * c_out_host != NULL and m >= 2: c_out_host[0] = cL = <a'[0, m/2), b'[m/2, m)>, c_out_host[1] = cR = <a'[m/2, m), b'[0, m/2)> of the
 * folded vectors, formed in the same pass; with m == 1 or c_out_host == NULL they are not computed and c_out_host is not written.
 * A thread owns j and j + m/2: it reads the four positions of a and of b that it alone writes or that nobody writes, so the
 * update needs no second buffer.  x is inverted once on the host.  Two launches with the inner products, one without.
 * ZKP_ERR_BAD_ARG: a NULL or misaligned a_dev / b_dev, n outside the rule, a and b overlapping, *x_host == 0 or >= r. */
int32_t zkp_fr_ipa_fold_ab_dev(zkp_ctx* ctx, zkp_curve_t curve, uint64_t* a_dev, uint64_t* b_dev, size_t n, const uint64_t* x_host,
                               uint64_t* c_out_host);
/* aSVC subvector commitments (later in 0.7.1, detected by symbol): the Fr work of asvc/src/lib.rs that no earlier entry covers.
 * `commit` is zkp_msm_g1_mont_dev over a resident Lagrange-basis key, prove_pos (:182-225) an inverse zkp_ntt_dev, the quotient
 * below and zkp_msm_g1_mont_dev over the powers of tau; the updates and aggregate_proofs are small variable-base MSMs.
 * The domain is the one of zkp_ntt_dev: n = 2^log_n, w its root of unity, 1 <= log_n <= min(30, two-adicity) (above:
 * ZKP_ERR_DOMAIN_TOO_LARGE).  positions_host: k distinct positions p_i < n, host memory, any order, 1 <= k <=
 * min(n, ZKP_ASVC_MAX_POSITIONS).  Vectors: Fr, Montgomery, canonical, 16-byte aligned, device memory.  Every element written is
 * the canonical Montgomery representative (bit-exact results).  Every argument is checked before anything runs: on an error every
 * output is untouched.
 *
 * The weights c_i = 1 / A_I'(w^p_i) = 1 / prod_{j != i} (w^p_i - w^p_j) of A_I(X) = prod_i (X - w^p_i), the coefficients of
 * aggregate_proofs (:425-431), in the order of positions_host: the k^2 differences are multiplied on the device (one workgroup per
 * position), then ONE batch inversion.  k == 1 gives 1.  At least one of weights_dev (k Fr) and weights_host (k Fr) is given; with
 * weights_host the call returns after the copy, otherwise it only launches.  Three launches.
 * ZKP_ERR_BAD_ARG: log_n == 0, k outside the rule, a position >= n, a repeated position, both outputs NULL, a misaligned weights_dev. */
#define ZKP_ASVC_MAX_POSITIONS 1024
int32_t zkp_fr_asvc_subset_weights_dev(zkp_ctx* ctx, zkp_curve_t curve, uint32_t log_n, const uint32_t* positions_host, size_t k,
                                       uint64_t* weights_dev, uint64_t* weights_host);
/* q = floor(Phi / A_I) (the divide_with_q_and_r of :197-212): phi_dev holds the n coefficients of Phi, q_dev receives the n - k
 * coefficients of the quotient; k == n writes nothing.  With w_i = w^p_i and the weights c_i above,
 *   q[t] = sum_i c_i S_i[t],   S_i[t] = Phi[t+1] + w_i S_i[t+1],  S_i[n-1] = 0:
 * k first-order suffix recurrences combined with k weights; the arithmetic is exact, so q equals long division bit for bit.
 * The recurrences are cut into segments of L = 2^floor(log2 k) coefficients.  Because sum_i c_i w_i^m = 0 for m < k - 1 and L <= k,
 * what a segment's own coefficients contribute cancels, and q[t] = sum_i c_i E_i[s] w_i^d with E_i[s] the value of S_i at the top of
 * t's segment s and d the distance of t below that top.  One pass forms the segment heads sum_j Phi[sL + j] w_i^j (four positions
 * share each coefficient load), a blocked suffix scan with the ratios w_i^L turns them into c_i E_i[s] in place (n k / L <= 2 n
 * elements of scratch, nothing of size n k), and one pass accumulates eight consecutive q[t] per thread over all positions in
 * registers and writes each once.  About 2 + 3 / L products per (coefficient, position).  Nine launches whatever k is; Phi is read
 * once per four positions (the re-reads hit the cache: all positions of a segment run side by side).  Launches only, like
 * zkp_fr_vec_op_dev.  ZKP_ERR_BAD_ARG: the rules above, a NULL or misaligned phi_dev / q_dev, q_dev overlapping phi_dev. */
int32_t zkp_fr_asvc_quotient_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* phi_dev, uint32_t log_n,
                                 const uint32_t* positions_host, size_t k, uint64_t* q_dev);
/* Matrix polynomial commitments over a resident Pedersen key (later in 0.7.1, detected by symbol): `packing_poly_commit` /
 * `poly_commit_vec` of hyrax, libra and spartan (spartan/src/commitments.rs:10-56, libra/src/evaluate.rs:130-170) and the row fold
 * of LogDotProductProof::reduce_prover (hyrax/src/commitment.rs:335-578).  BN254 / BLS12-381 G1.  The logarithmic argument after
 * the fold is zkp_g1_ipa_fold_dev + zkp_msm_g1_var_batch_dev; the transcript, the blinds and the challenges stay with the caller.
 *
 * The key: n_gens generators (`gen_n` of PolyCommitmentSetupParameters) and the blinding generator h, affine Montgomery points in
 * HOST memory in the layout of zkp_bases_upload_g1; gens_inf_host: identity flags or NULL (= none); a (0, 0) point is an identity
 * too, and an identity stays one at every level.  1 <= n_gens <= ZKP_PEDERSEN_MAX_GENS (== ZKP_MSM_SMALL_MAX_G1, so every round of
 * the inner-product argument that follows stays inside the batch MSM's cap).  The key holds the window tables 2^(c w) g_j, w < W =
 * floor((256 + c) / c), as affine points in device memory (h is generator n_gens): W (n_gens + 1) points of 64 / 96 bytes, c = 8.
 * Creation is one-time work, exact, 2 W launches (c doublings per level in registers, one batch inversion per 64 points and level);
 * it runs on the context's current stream, takes scratch from the context's grow-only arena and returns when the tables are
 * built.  ZKP_ERR_BAD_ARG: a NULL gens_xy_host / h_xy_host / out, n_gens outside the rule; ZKP_ERR_OOM: the tables do not fit;
 * on an error *out is untouched.  A key belongs to the context that created it; zkp_pedersen_key_free waits for that context's
 * current stream first.
 * zkp_pedersen_key_info: info[0] n_gens, [1] c, [2] W, [3] (generator, window) pairs per slice at most (G W with G = floor(4096 / W)
 * generators), [4] table bytes, [5] LDS bytes of one workgroup of the bucket pass, [6] launches per commitment call, [7] 0. */
#define ZKP_PEDERSEN_MAX_GENS 65536
typedef struct zkp_pedersen_key zkp_pedersen_key;
int32_t zkp_pedersen_key_create(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* gens_xy_host, const uint8_t* gens_inf_host,
                                size_t n_gens, const uint64_t* h_xy_host, zkp_pedersen_key** out);
int32_t zkp_pedersen_key_free(zkp_ctx* ctx, zkp_pedersen_key* key);
int32_t zkp_pedersen_key_info(const zkp_pedersen_key* key, uint64_t* info);
/* out[i] = (sum_{j < cols} scalars[i cols + j] g_j + blinds[i] h).into_affine() for i < rows; blinds_dev == NULL: no blind term.
 * rows == 1 is poly_commit_vec.  scalars_dev: rows x cols Fr, row-major; blinds_dev: rows Fr; both Montgomery (into_repr() fused),
 * 16-byte aligned, device memory.  out_xy_dev: rows affine Montgomery points (16-byte aligned), out_inf_dev: rows flags, device
 * memory; every point is the canonical affine form (bit-exact results) and an identity is written exactly as
 * zkp_fixed_base_mul_g1 writes it (words and flag).  rows >= 1, 1 <= cols <= n_gens, rows * cols <= 2^28.
 * Three launches whatever rows and cols are, no host loop over rows: one wave per (row, slice of <= G generators) walks every
 * scalar's W signed window digits once, sorts the <= 4096 (generator, window) pairs by bucket (stable counting sort in LDS) and
 * accumulates them into 2^(c-1) LDS buckets conflict-free and in a fixed order, then reduces sum_b (b + 1) B_b — the tables carry
 * the window weights, so there is no doubling tail; one wave per row adds the slices and the blind term; one lane per row
 * converts to affine with one inversion per 64 rows.  All additions are complete (equal, opposite and identity operands).
 * ZKP_ERR_BAD_ARG: a NULL key / scalars_dev / out_xy_dev / out_inf_dev, a key of another context, a misaligned scalars_dev /
 * blinds_dev / out_xy_dev, rows or cols outside the rules, an output overlapping an input or the other output.  Scratch:
 * rows * (ceil(cols / G) + 1) bucket points (144 / 224 bytes) from the context's grow-only arena (ZKP_ERR_OOM if it cannot grow).
 * Every argument is checked before anything runs: on an error the outputs are untouched.  Runs on the context's current stream;
 * launches only, like zkp_fr_vec_op_dev. */
int32_t zkp_pedersen_commit_rows_dev(zkp_ctx* ctx, const zkp_pedersen_key* key, const uint64_t* scalars_dev, size_t rows, size_t cols,
                                     const uint64_t* blinds_dev, uint64_t* out_xy_dev, uint8_t* out_inf_dev);
/* out[j] = sum_{i < rows} l[i] m[i cols + j] for j < cols: the row fold lz = L^T M of reduce_prover.  l_dev: rows Fr, m_dev:
 * rows x cols Fr row-major, out_dev: cols Fr; Montgomery, canonical, 16-byte aligned, device memory; every element written is the
 * canonical Montgomery representative.  rows >= 1, cols >= 1, rows * cols <= 2^28; out_dev overlaps neither input.
 * Lanes take consecutive columns (coalesced loads), a workgroup ZKP_FR_VECMAT_ROW_CHUNK rows; with more than one chunk the partial
 * sums go to the context's grow-only arena (32 * cols * ceil(rows / ZKP_FR_VECMAT_ROW_CHUNK) bytes) and a second launch adds them
 * in chunk order: two launches at most.  ZKP_ERR_BAD_ARG: a NULL or misaligned pointer, a shape outside the rules, out_dev
 * overlapping l_dev or m_dev.  Every argument is checked before anything runs: on an error out_dev is untouched.  Runs on the
 * context's current stream; launches only. */
#define ZKP_FR_VECMAT_ROW_CHUNK 32
int32_t zkp_fr_vecmat_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* l_dev, const uint64_t* m_dev, size_t rows, size_t cols,
                          uint64_t* out_dev);
/* Transforms over G1 points (later in 0.7.1, detected by symbol): the primitive behind all n single-position aSVC proofs in
 * O(n log n) (Tomescu et al. §3.4, after Feist-Khovratovich) and behind a Lagrange-form KZG / aSVC key from the powers of tau
 * without the trapdoor.  BN254 / BLS12-381 G1.  Points: affine Montgomery words + identity flags in DEVICE memory, the layout of
 * zkp_g1_ipa_fold_dev (16-byte aligned); a (0, 0) point is an identity too.  Every point written is the canonical affine
 * Montgomery representative (bit-exact results), and an identity is written exactly as zkp_fixed_base_mul_g1 writes it (words and
 * flag).  All additions are complete (equal, opposite and identity operands).  Every argument is checked before anything runs: on
 * an error the buffers are untouched.  Both calls only launch, on the context's current stream, like zkp_fr_vec_op_dev: no host
 * work proportional to n, no device-to-host copy.
 *
 * out[i] = [s_i] P_i for i < n.  inf_dev: identity flags or NULL (= none).  scalars_dev: n Fr, Montgomery, canonical, 16-byte
 * aligned, device memory.  out_xy_dev may equal xy_dev and out_inf_dev may equal inf_dev (in place); any other overlap of an output
 * with an input or the other output -> ZKP_ERR_BAD_ARG.  n == 0 -> ZKP_OK, nothing runs.  One launch: one lane per point; the lane
 * reads its own scalar, recodes it into signed fixed windows and keeps its window table in LDS; one batch inversion per 64 points.
 * ZKP_ERR_BAD_ARG: a NULL xy_dev / scalars_dev / out_xy_dev / out_inf_dev, a misaligned pointer, n > 2^31, a curve without G1
 * support here. */
int32_t zkp_g1_scale_vec_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy_dev, const uint8_t* inf_dev,
                             const uint64_t* scalars_dev, size_t n, uint64_t* out_xy_dev, uint8_t* out_inf_dev);
/* In place over 2^log_n points, natural order in and out.  op = ZKP_NTT_FFT: out[i] = sum_j [w^(i j)] P_j;
 * op = ZKP_NTT_IFFT: out[i] = [1/n] sum_j [w^(-i j)] P_j, with w the root zkp_ntt_dev uses for the same log_n.
 * 1 <= log_n <= ZKP_G1_NTT_MAX_LOG.  inf_dev is required: outputs can be identities whatever the inputs are.
 * log_n + 2 launches (the twiddle table, the bit reversal, one per stage; the stage of twiddle 1 multiplies nothing), one more for
 * the 1 / n of the inverse; one lane per butterfly (P, Q) -> (P + [w] Q, P - [w] Q), every stage ends in affine form.  The n / 2
 * twiddles live in the context's grow-only scratch.
 * ZKP_ERR_BAD_ARG: a NULL or misaligned xy_dev, a NULL inf_dev, inf_dev inside xy_dev, log_n outside the rule, any other op, a curve
 * without G1 support here. */
#define ZKP_G1_NTT_MAX_LOG 24
int32_t zkp_g1_ntt_dev(zkp_ctx* ctx, zkp_curve_t curve, uint64_t* xy_dev, uint8_t* inf_dev, uint32_t log_n, int32_t op);
/* Algebraic hashes and complete binary Merkle trees (later in 0.7.1, detected by symbol): the `*_block` / `*_hash` functions of
 * gadgets/src/hashes/{mimc,poseidon,rescue}.rs and the tree of gadgets/src/merkletree/cbmt.rs, i.e. the values that the reference's
 * hash and membership circuits (cli/src/circuits/hash.rs, gadgets/src/merkletree/cbmt_constraints.rs, marlin/examples/mimc.rs)
 * assign.  The producer of a device-resident witness for zkp_groth16_prove_dev.  Fr of BN254 / BLS12-381; state width
 * ZKP_HASH_WIDTH = 3 (rate 2, capacity 1), the reference's M.  The library ships NO constant table: every round constant, matrix
 * and exponent is the caller's (the reference's Poseidon / Rescue tables are literals of its source, its MiMC constants come from
 * a seeded generator).
 *
 * zkp_hash_desc: the parameters of one hash.  Field elements: Fr, Montgomery, < r, HOST memory, 4 x u64 each.
 *   ZKP_HASH_MIMC      rounds 1..ZKP_HASH_MAX_ROUNDS_MIMC; constants[rounds].  The block is mimc_block (mimc.rs:49-62): per round
 *                      t = xl + c_i, (xl, xr) <- (t^3 + xr, xl); the result is xl.  alpha, mds, full_round, inv_alpha: ignored.
 *   ZKP_HASH_POSEIDON  rounds 1..ZKP_HASH_MAX_ROUNDS_POSEIDON; alpha 3, 5 or 7; constants = ark[rounds][3]; mds[3][3] row-major;
 *                      full_round[rounds], one byte per round (0 = partial).  The block is poseidon_block (poseidon.rs:553-585):
 *                      state (xl, xr, 0); per round state += ark[i], x^alpha on all three elements (full) or on element 2 only
 *                      (partial), state <- mds state; the result is state[0].  The per-round flag expresses both the reference's
 *                      schedule (:560 makes exactly round RF / 2 partial) and the standard RF / 2 full, RP partial, RF / 2 full.
 *   ZKP_HASH_RESCUE    rounds R 1..ZKP_HASH_MAX_ROUNDS_RESCUE; alpha 3, 5 or 7; inv_alpha: a plain 256-bit integer, little-endian
 *                      words, not zero; constants[2 R + 1][3]; mds[3][3].  The block is rescue_block (rescue.rs:337-367): state
 *                      (xl, xr, 0) + constants[0]; for i < 2 R: x^alpha (i even) or x^inv_alpha (i odd) on all three elements,
 *                      state <- mds state + constants[i + 1]; the result is state[0].  At creation a one-lane kernel checks
 *                      (x^alpha)^inv_alpha == x for the fixed x = 2, 3 (and 5): a mismatch -> ZKP_ERR_BAD_ARG and no handle.
 * zkp_hash_params_create copies the constants once to device memory the handle owns, on the context's current stream, and returns
 * when they are there.  A handle belongs to the context that created it: every entry that is given one of another context returns
 * ZKP_ERR_BAD_ARG; zkp_hash_params_free waits for that context's current stream first.  ZKP_ERR_BAD_ARG: struct_size smaller than
 * the struct, an unknown kind, rounds or alpha out of range, a NULL table the kind needs, an element >= r, inv_alpha == 0, the
 * Rescue check; on an error *out is untouched.
 * zkp_hash_params_info: info[0] kind, [1] curve, [2] rounds, [3] device bytes held, [4] alpha (0 for MiMC), [5] Fr products of one
 * block by the schedule, [6] and [7] 0. */
#define ZKP_HASH_WIDTH 3
#define ZKP_HASH_MAX_ROUNDS_MIMC 512
#define ZKP_HASH_MAX_ROUNDS_POSEIDON 128
#define ZKP_HASH_MAX_ROUNDS_RESCUE 64
#define ZKP_HASH_MAX_LOG_BLOCKS 28
#define ZKP_HASH_MAX_LOG_LEAVES 27
typedef enum { ZKP_HASH_MIMC = 0, ZKP_HASH_POSEIDON = 1, ZKP_HASH_RESCUE = 2 } zkp_hash_kind;
typedef enum { ZKP_MERGE_BLOCK = 0, ZKP_MERGE_CHAIN = 1 } zkp_merge;
typedef struct {
  uint32_t struct_size;        /* sizeof(zkp_hash_desc) as the caller compiled it */
  int32_t kind;                /* zkp_hash_kind */
  uint32_t rounds;
  uint32_t alpha;
  const uint64_t* constants;   /* MiMC: rounds; Poseidon: rounds x 3; Rescue: (2 rounds + 1) x 3 */
  const uint64_t* mds;         /* 3 x 3, row-major (Poseidon, Rescue) */
  const uint8_t* full_round;   /* rounds bytes (Poseidon) */
  uint64_t inv_alpha[4];       /* (Rescue) */
} zkp_hash_desc;
typedef struct zkp_hash_params zkp_hash_params;
int32_t zkp_hash_params_create(zkp_ctx* ctx, zkp_curve_t curve, const zkp_hash_desc* desc, zkp_hash_params** out);
int32_t zkp_hash_params_free(zkp_ctx* ctx, zkp_hash_params* params);
int32_t zkp_hash_params_info(const zkp_hash_params* params, uint64_t* info);
/* The batched permutations: one lane per block, the whole permutation in registers, the constants through wave-uniform loads.
 * Vectors: Fr, Montgomery, canonical, 16-byte aligned, DEVICE memory; every element written is the canonical Montgomery
 * representative (bit-exact results).  Every argument is checked before anything runs: on an error the outputs are untouched.
 * All of them run on the context's current stream and only launch, like zkp_fr_vec_op_dev: no host work proportional to n.
 *
 * out[k] = block(xl[k], xr[k]) for k < n, 1 <= n <= 2^ZKP_HASH_MAX_LOG_BLOCKS.  out_dev may be xl_dev or xr_dev itself; any other
 * overlap of out with an input -> ZKP_ERR_BAD_ARG.  One launch. */
int32_t zkp_fr_hash_blocks_dev(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* xl_dev, const uint64_t* xr_dev, size_t n,
                               uint64_t* out_dev);
/* The reference's `*_hash` (mimc.rs:78-90, poseidon.rs:601-613, rescue.rs:383-395) over n messages of len elements each, row-major
 * in msgs_dev: h = 0, then h <- block(h, m[k len + j]) for j < len; out[k] is the image and xl_out[k] (xl_out_dev may be NULL) is h
 * before the last block, the `xl` that the gadget allocates (`*_hash` returns (xl, xr, image); xr is the last message element).
 * n >= 1, len >= 1, n len <= 2^ZKP_HASH_MAX_LOG_BLOCKS.  The outputs overlap neither the messages nor each other.  One launch. */
int32_t zkp_fr_hash_chain_dev(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* msgs_dev, size_t n, size_t len,
                              uint64_t* out_dev, uint64_t* xl_out_dev);
/* MiMC only (another kind -> ZKP_ERR_BAD_ARG): the auxiliary assignment of the `mimc` gadget (mimc.rs:110-157) in its allocation
 * order.  For block k, 2 rounds + 2 elements at out + k stride: xl, xr, then per round tmp_i = (xl_i + c_i)^2 and new_xl_i.
 * 1 <= n <= 2^ZKP_HASH_MAX_LOG_BLOCKS, stride >= 2 rounds + 2, n stride <= 2^32; the elements of a gap between two blocks are not
 * written.  out overlaps neither input.  With 5 rounds and stride 12 at z_dev + 32 bytes this is the whole auxiliary assignment of
 * marlin/examples/mimc.rs.  One launch. */
int32_t zkp_fr_mimc_trace_dev(zkp_ctx* ctx, const zkp_hash_params* params, const uint64_t* xl_dev, const uint64_t* xr_dev, size_t n,
                              uint64_t* out_dev, size_t stride);
/* The complete binary Merkle tree of cbmt.rs (:182-202): nodes_dev holds 2 n - 1 Fr with the n leaves already at [n - 1, 2 n - 1);
 * the call fills [0, n - 1) with nodes[i] = merge(nodes[2 i + 1], nodes[2 i + 2]); nodes[0] is the root.  Any 1 <= n <=
 * 2^ZKP_HASH_MAX_LOG_LEAVES, not only powers of two; n == 1 launches nothing.  merge: ZKP_MERGE_BLOCK = block(l, r);
 * ZKP_MERGE_CHAIN = block(block(0, l), r), the reference's hash(l || r) (MergeMimc, cbmt_constraints.rs:146-155).
 * With depth(i) = floor(log2(i + 1)) and D = depth(n - 2): one launch per depth D, ..., 9, one lane per node, then ONE workgroup of
 * 256 lanes for the depths 8 .. 0 with a barrier between them: max(0, D - 8) + 1 launches. */
int32_t zkp_fr_merkle_tree_dev(zkp_ctx* ctx, const zkp_hash_params* params, int32_t merge, uint64_t* nodes_dev, size_t n);
/* build_proof (cbmt.rs:31-72) for q leaves at once: for leaf_idx_dev[k] (uint32, device memory, any order, repeats allowed) the
 * siblings from heap index n - 1 + leaf upwards, the root excluded, go to out + k stride and their count, depth(n - 1 + leaf), to
 * len_dev[k]; the elements from the count up to stride are zeroed.  stride >= depth(2 n - 2); n == 1 gives length 0.  A leaf
 * index >= n gives len_dev[k] = ZKP_MERKLE_BAD_LEAF and a zeroed row, and reads nothing outside nodes_dev.  1 <= n <=
 * 2^ZKP_HASH_MAX_LOG_LEAVES, 1 <= q <= 2^ZKP_HASH_MAX_LOG_BLOCKS, q max(stride, 1) <= 2^32.  The outputs overlap neither the inputs
 * nor each other.  One gather launch, no arithmetic: the curve does not enter.
 * ZKP_ERR_BAD_ARG of the five entries above: a NULL or misaligned pointer (leaf_idx_dev / len_dev: 4 bytes), a count of 0 or above
 * its cap, a stride too small, an unknown merge, a params handle of another context or (trace) of another kind, spans that overlap
 * against the rules. */
#define ZKP_MERKLE_BAD_LEAF 4294967295u
int32_t zkp_fr_merkle_paths_dev(zkp_ctx* ctx, const uint64_t* nodes_dev, size_t n, const uint32_t* leaf_idx_dev, size_t q,
                                uint64_t* out_dev, size_t stride, uint32_t* len_dev);
/* SHA-256 and the witness of bit circuits (later in 0.7.1, detected by symbol): the byte hash behind the reference's sha256 gadget
 * (gadgets/src/hashes/sha256.rs) and its Merkle-membership example (gadgets/examples/merkle_tree_sha256.rs), and the producer of
 * that circuit's device-resident witness for zkp_groth16_prove_dev.  No field arithmetic: the curve enters the last entry only.
 * Pointers are DEVICE memory, 16-byte aligned.  Every argument is checked before anything runs: on an error the outputs are
 * untouched.  All of them run on the context's current stream and only launch: no host work proportional to n.
 *
 * The canonical trace of n messages of len bytes is uint32 T[w n + k], word w < W, message k < n, with
 * W = 1 + ZKP_SHA256_BLOCK_WORDS ceil((len + 9) / 64).  Word 0 is 0.  Block b of the padded message owns the ZKP_SHA256_BLOCK_WORDS
 * words from 1 + ZKP_SHA256_BLOCK_WORDS b, at the offsets that zkp_sha256_info reports:
 *   input + j, j < 16             the block's input words, as SHA-256 reads them
 *   sched + 6 (i - 16), i = 16..63  rotr7 ^ rotr18 of w[i-15]; that ^ shr3; rotr17 ^ rotr19 of w[i-2]; that ^ shr10; the integer
 *                                 w[i-16] + s0 + w[i-7] + s1 as lo, hi
 *   round + 11 i, i < 64          the integer that forms the round's e as lo, hi; rotr6 ^ rotr11 of e; that ^ rotr25; ch; the integer
 *                                 that forms the round's a as lo, hi; rotr2 ^ rotr13 of a; that ^ rotr22; maj; b & c.  In round 0 the
 *                                 two integers are the incoming state words, hi = 0
 *   final + 2 k, k < 8            the integer h_k as lo, hi; h0 and h4 fold the operands that round 63 deferred (8 and 7 operands)
 * The integers are the full sums, not reduced mod 2^32: the gadget allocates their carry bits (uint32.rs:285-357).
 *
 * zkp_sha256_info: info[16] = words per block, input offset, sched offset, words per sched record, round offset, words per round
 * record, final offset, ZKP_SHA256_MAX_LOG_LEN, _BYTES, _TRACE_WORDS, _LEAVES, _CODE_WORDS, the lanes of a hashing workgroup, the
 * lanes of an expanding workgroup, 0, 0. */
#define ZKP_SHA256_BLOCK_WORDS 1024
#define ZKP_SHA256_MAX_LOG_LEN 20
#define ZKP_SHA256_MAX_LOG_BYTES 34
#define ZKP_SHA256_MAX_LOG_TRACE_WORDS 32
#define ZKP_SHA256_MAX_LOG_LEAVES 27
#define ZKP_SHA256_MAX_LOG_CODE_WORDS 26
int32_t zkp_sha256_info(uint64_t* info);
/* out[32 k, 32 k + 32) = SHA-256 of the len bytes at msgs + k len, in digest byte order.  0 <= len <= 2^ZKP_SHA256_MAX_LOG_LEN,
 * n >= 1, n (len + 1) <= 2^ZKP_SHA256_MAX_LOG_BYTES.  The messages are not written; out overlaps them nowhere.  One launch, one
 * lane per message. */
int32_t zkp_sha256_dev(zkp_ctx* ctx, const uint8_t* msgs_dev, size_t n, size_t len, uint8_t* out_dev);
/* The canonical trace of the same n messages: W n words to trace_dev.  The rules of zkp_sha256_dev, and
 * W n <= 2^ZKP_SHA256_MAX_LOG_TRACE_WORDS.  One launch. */
int32_t zkp_sha256_trace_dev(zkp_ctx* ctx, const uint8_t* msgs_dev, size_t n, size_t len, uint32_t* trace_dev);
/* The complete binary Merkle tree of cbmt.rs:182-202 over 32-byte items with merge(l, r) = SHA-256(l || r): nodes_dev holds 2 n - 1
 * items with the n leaves already at [n - 1, 2 n - 1); the call fills [0, n - 1); nodes[0] is the root.  Any 1 <= n <=
 * 2^ZKP_SHA256_MAX_LOG_LEAVES; n == 1 launches nothing.  One launch per depth of inner nodes, one lane per node, two compressions
 * per lane.  Membership paths need no entry of their own: zkp_fr_merkle_paths_dev is a gather of 32-byte nodes without arithmetic
 * and serves such a tree as it stands. */
int32_t zkp_sha256_merkle_tree_dev(zkp_ctx* ctx, uint8_t* nodes_dev, size_t n);
/* The witness of a bit circuit from a trace: z[b z_stride + j] = bit ^ neg for b < q, j < m, as zero or the Montgomery one of
 * `curve`, where code_dev[j] = v << 6 | bit << 1 | neg (uint32) selects bit `bit` of word v % words_per_msg of message
 * v / words_per_msg of instance b, and trace_dev is the trace of q msgs_per_instance messages, those of instance b at
 * [b msgs_per_instance, (b + 1) msgs_per_instance).  Code 0 is the constant 0 and code 1 the constant 1 (word 0 of a trace is 0).
 * max_v: the largest v among the codes, which the CALLER states (a driver computes it once, when it uploads the codes);
 * max_v >= words_per_msg msgs_per_instance -> ZKP_ERR_BAD_ARG.  The codes themselves are not read on the host; a code whose v lies
 * outside the instance's words although max_v said otherwise reads nothing and gives its bare neg.  words_per_msg msgs_per_instance <= 2^ZKP_SHA256_MAX_LOG_CODE_WORDS, that times q <= 2^ZKP_SHA256_MAX_LOG_TRACE_WORDS,
 * q >= 1, m >= 1, z_stride >= m, q z_stride <= 2^32; the elements of a gap between two instances are not written.  z overlaps
 * neither input.  One launch, 32 bytes per lane in two 16-byte stores.  The entry knows nothing of SHA-256: any bit circuit whose
 * values are bits of a word-major trace can use it.
 * ZKP_ERR_BAD_ARG of the four entries above: a NULL or misaligned pointer, a count of 0 or above its cap, a stride too small,
 * spans that overlap against the rules; ZKP_ERR_UNSUPPORTED_CURVE: another curve. */
int32_t zkp_fr_bits_expand_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint32_t* trace_dev, size_t words_per_msg, size_t msgs_per_instance,
                               size_t q, const uint32_t* code_dev, size_t m, uint32_t max_v, uint64_t* z_dev, size_t z_stride);
/* Optimal-ate pairings (later in 0.7.1, detected by symbol): products of Miller functions and the final exponentiation on BN254 and
 * BLS12-381, the primitive of groth16::verify_proof (groth16/src/verifier.rs:8-44), KZG10::check (marlin/src/pc/kzg10.rs:158-173)
 * and the aSVC checks.  n pairs (P_i, Q_i) form m = n / group groups of `group` consecutive pairs; a group's value is the product of
 * its pairs' Miller functions, and checking it costs ONE final exponentiation.
 *
 * Points: the layouts of zkp_msm_g1_var / zkp_msm_g2_var, affine Montgomery words (G1: x, y; G2: x.c0, x.c1, y.c0, y.c1) plus one
 * identity flag byte per point; both flag arrays are required.  A pair with a flagged point contributes 1.  The entries do NOT test
 * curve or subgroup membership: callers use zkp_g1_subgroup_check / zkp_g2_subgroup_check (a point off the curve gives a value
 * without meaning, never a fault).
 * An Fq12 is 12 Fq, Montgomery, in ark's tower order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, each an Fq2 (c0, c1), over
 * Fq12 = Fq6[w] / (w^2 - v), Fq6 = Fq2[v] / (v^3 - xi), xi = 9 + u (BN254) / 1 + u (BLS12-381): c_j.c_i is the coefficient of
 * w^(2 i + j).  48 / 72 u64 words.  Every element written is fully reduced (< q): equality of GT values is equality of words.
 * The final exponentiation returns f^(k (q^12 - 1) / r) for a per-curve constant k coprime to r, fixed at compile time: k = 1 on
 * BN254, k = 3 on BLS12-381.  A pairing value is therefore e(P, Q)^k: bilinear, non-degenerate, comparable with other values of this
 * library only.  An input of 0 gives 0 (Fq's inversion maps 0 to 0); the Miller function of valid points is never 0.
 *
 * zkp_pairing_info: info[0] k, [1] u64 words per Fq12, [2] pairs per workgroup, [3] ZKP_PAIRING_MAX_N, [4] LDS bytes of the Miller
 * kernel, [5..7] 0.  Needs no device.
 * zkp_pairing_miller_dev: out[j] = the product over the pairs of group j of the optimal-ate Miller function, m Fq12; defined up to
 * factors that the final exponentiation removes.  One pair per lane; the pairs of a group are multiplied in a tree over the wave in
 * LDS, and a second launch joins the parts of a group that spans workgroups.  Two launches; one, and no scratch, when `group`
 * divides 64 (no group spans workgroups).
 * zkp_pairing_final_exp_dev: out[e] = final_exp(f[e]) for e < m, one element per lane, one launch.  out_gt_dev may be f12_dev itself
 * (in place); any other overlap is refused.
 * zkp_pairing_product_is_one_dev: both steps, then ok_dev[j] = 1 iff group j's GT value is one, else 0; m bytes.  Four launches (three when `group` divides 64).
 * The three *_dev entries run on the context's current stream and only launch; intermediate values live in the context's grow-only
 * scratch.
 * zkp_pairing: HOST pointers; gt_out[i] = e(P_i, Q_i)^k for i < n, n Fq12.  zkp_pairing_check: HOST pointers; ok_out[j] as above.
 * Both stage, run and synchronise.
 * ZKP_ERR_BAD_ARG, before anything runs and with every output untouched: a NULL pointer, a point or Fq12 pointer in device memory
 * that is not 16-byte aligned, n, m or group == 0, n not a multiple of group, n or m above ZKP_PAIRING_MAX_N, an unknown curve, an
 * output that overlaps an input (but for the in-place case above). */
#define ZKP_PAIRING_MAX_N 1048576
int32_t zkp_pairing_info(zkp_curve_t curve, uint64_t* info);
int32_t zkp_pairing_miller_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* g1_xy_dev, const uint8_t* g1_inf_dev,
                               const uint64_t* g2_xy_dev, const uint8_t* g2_inf_dev, size_t n, size_t group, uint64_t* out_f12_dev);
int32_t zkp_pairing_final_exp_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* f12_dev, size_t m, uint64_t* out_gt_dev);
int32_t zkp_pairing_product_is_one_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* g1_xy_dev, const uint8_t* g1_inf_dev,
                                       const uint64_t* g2_xy_dev, const uint8_t* g2_inf_dev, size_t n, size_t group, uint8_t* ok_dev);
int32_t zkp_pairing(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                    const uint8_t* g2_inf, size_t n, uint64_t* gt_out);
int32_t zkp_pairing_check(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* g1_xy, const uint8_t* g1_inf, const uint64_t* g2_xy,
                          const uint8_t* g2_inf, size_t n, size_t group, uint8_t* ok_out);
/* PLONK prover rounds 2 and 3 (later in 0.7.1, detected by symbol): the table work of AHPForPLONK::prover_second_round /
 * prover_third_round (plonk/src/ahp/prover.rs:135-216), every table kept on the device.  The transforms around them are
 * zkp_ntt_dev, the commitments zkp_msm_g1_mont_dev; the transcript stays with the caller.  Vectors: Fr, Montgomery, canonical,
 * 16-byte aligned, device memory.  Scalars (*_host): Fr, Montgomery, < r, host memory.
 *
 * The exclusive running product:  out[0] = 1, out[i] = in[0] * ... * in[i-1]  for i < n;  *total_out_host (may be NULL) receives
 * in[0] * ... * in[n-1].  1 <= n <= 2^30, any n.  out_dev may be in_dev itself; otherwise the two must not overlap.
 * A workgroup owns a block of 1024 consecutive elements.  n <= 1024: one launch.  More: one launch leaves every block's total, the
 * totals are scanned the same way (one more level per factor of 1024), one launch replays every block from its scanned total:
 * 3 launches up to 2^20 elements, 5 above.  Separate launches on the context's stream: no kernel waits for another workgroup.
 * ZKP_ERR_BAD_ARG, before anything runs: a NULL or misaligned vector, n outside the rule, vectors that overlap in part.
 * Every element written is the canonical Montgomery representative (bit-exact results). */
int32_t zkp_fr_prefix_product_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* in_dev, uint64_t* out_dev, size_t n,
                                  uint64_t* total_out_host);
/* PermutationKey::compute_z (plonk/src/ahp/indexer/permutation.rs:67-118) up to the evaluation vector z over domain_n, n = 2^log_n:
 *   perm[i] = prod_j (w_j[i] + ks_j beta w^i + gamma) / prod_j (w_j[i] + beta sigma_j[i] + gamma),   z[0] = 1, z[i+1] = z[i] perm[i]
 * with w = domain_n.element(1), the root zkp_ntt_dev uses for log_n.  w_dev / sigma_dev: host arrays of 4 device pointers to n Fr
 * each (w_0..w_3 = aux, l, r, o of composer/arithmetic.rs; sigma_0..sigma_3 of composer/permutation.rs:62-83); ks_host: 4 Fr.
 * The n inversions are ONE batch inversion (zkp_fr_batch_inverse_dev's kernel and convention: a zero denominator inverts to
 * zero, where the reference panics at :99), the products zkp_fr_prefix_product_dev's launches over num[i] * (1 / den)[i].
 * *closes_out_host = 1 when z[n-1] perm[n-1] == 1 (the assert_eq! of :112), else 0; the call returns ZKP_OK either way.
 * Only z_out_dev[0 .. n) is written, last and from scratch memory: it may be one of the inputs.
 * ZKP_ERR_BAD_ARG, before anything runs: a NULL or misaligned pointer, log_n < 2, a scalar >= r.  ZKP_ERR_DOMAIN_TOO_LARGE:
 * log_n + 2 above the field's two-adicity (the 4n domain of the third round, PolynomialDegreeTooLarge). */
int32_t zkp_fr_plonk_perm_z_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* const* w_dev, const uint64_t* const* sigma_dev,
                                uint32_t log_n, const uint64_t* ks_host, const uint64_t* beta_host, const uint64_t* gamma_host,
                                uint64_t* z_out_dev, int32_t* closes_out_host);
/* The third-round quotient over the N = 4n points x_i = g w^i of the coset that ZKP_NTT_COSET_FFT evaluates on (g its coset
 * generator, w = domain_4n.element(1)), ONE pass and one launch (prover.rs:184-202):
 *   t[i] = (t_arith[i] + t_perm[i]) * v_4n_inversed[i]
 *   t_arith[i] = (q_0 w_0 + q_1 w_1 + q_2 w_2 + q_3 w_3 + q_m w_1 w_2 + q_c + pi)[i] * q_arith[i]       (indexer/arithmetic.rs:107-114;
 *                the q_arith.is_zero() branch is this product)
 *   t_perm[i]  = (prod_j (w_j[i] + ks_j beta x_i + gamma) z[i] - prod_j (w_j[i] + beta sigma_j[i] + gamma) z[(i + 4) mod N]) alpha
 *                + (z[i] - 1) l1[i] alpha^2                                                              (indexer/permutation.rs:155-166)
 *   v_4n_inversed[i] = 1 / (x_i^n - 1) = 1 / (g^n (w^n)^(i mod 4) - 1): four values, computed on the host   (indexer/mod.rs:223-225)
 * x_i (linear_4n, permutation.rs:134-137) is computed in the kernel.  w_4n / sigma_4n: host arrays of 4 device pointers, q_4n of
 * 7 in the order q_0, q_1, q_2, q_3, q_m, q_c, q_arith; every table N Fr.  18 table reads and one write per point.
 * t_out_dev must not overlap any input (point i + 4 of z is read by another thread than the one that writes point i).
 * ZKP_ERR_BAD_ARG, before anything runs: a NULL or misaligned pointer, log_n < 2, a scalar >= r, t_out_dev overlapping an input.
 * ZKP_ERR_DOMAIN_TOO_LARGE: log_n + 2 above the field's two-adicity. */
int32_t zkp_fr_plonk_quotient_dev(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* const* w_4n, const uint64_t* z_4n,
                                  const uint64_t* pi_4n, const uint64_t* const* q_4n, const uint64_t* const* sigma_4n,
                                  const uint64_t* l1_4n, uint32_t log_n, const uint64_t* ks_host, const uint64_t* beta_host,
                                  const uint64_t* gamma_host, const uint64_t* alpha_host, uint64_t* t_out_dev);
/* PLONK evaluations and opening polynomials (later in 0.7.1, detected by symbol): what Plonk::prove (plonk/src/lib.rs:93-204)
 * does with the coefficient vectors of rounds 1-3.  Rules common to both entries: 1 <= count <= 32; p_dev and ns are host arrays
 * of `count` device pointers and lengths; every ns[k] <= 2^30; ns[k] == 0 is the zero polynomial and its pointer may be NULL.
 * Vectors: Fr, Montgomery, canonical, 16-byte aligned, device memory.  Scalars (*_host): Fr, Montgomery, < r, host memory.
 * Every element written is the canonical Montgomery representative (bit-exact results); inputs are never written.
 * ZKP_ERR_BAD_ARG is returned before anything runs and with every output untouched.
 *
 * out_host[k] = sum_{i < ns[k]} p_k[i] z^i  for `count` polynomials at ONE point z (EvaluationsProvider::get_lc_eval,
 * plonk/src/ahp/evaluations.rs:24-49, one label at a time); out_host: count Fr.  The same pointer may appear more than once.
 * One pass reads every coefficient once with consecutive 16-byte loads: thread j of T = 256 * min(ceil(max ns / 256), 512)
 * owns the indices j, j + T, ..., forms z^j once and steps by z^T; the polynomials are walked in register groups of 4.
 * Two launches (the pass, then one workgroup per polynomial adds its partials), one copy back, one synchronise: the call
 * returns after the evaluations are on the host.  z == 0 gives p_k[0].
 * ZKP_ERR_BAD_ARG: count outside the rule, a length above 2^30, a NULL or misaligned vector with ns[k] > 0, *z_host >= r. */
int32_t zkp_fr_poly_eval_many_dev(zkp_ctx* ctx, zkp_curve_t curve, size_t count, const uint64_t* const* p_dev, const size_t* ns,
                                  const uint64_t* z_host, uint64_t* out_host);
/* out[i] = sum_{k : i < ns[k]} c_k p_k[i],  i < n_out   (the polynomial of an ark_poly_commit LinearCombination); coeffs_host:
 * count Fr.  One element-wise launch; the scalars and the pointer / length table travel as kernel arguments.  A term whose
 * scalar is zero (or whose length is 0) is dropped on the host; if every term is dropped, out is zero-filled.  1 <= n_out <= 2^30
 * and every ns[k] <= n_out.  out_dev may be one of the p_dev[k] itself (same base: index i is read before it is written and no
 * other index is touched); any other overlap of out_dev[0 .. n_out) with p_dev[k][0 .. ns[k]) is rejected.
 * Launches only, like zkp_fr_vec_op_dev: the result is ordered before later work on the context's stream.
 * ZKP_ERR_BAD_ARG: count or n_out outside the rule, ns[k] > n_out, a NULL or misaligned vector, out_dev overlapping an input
 * in part, a scalar >= r. */
int32_t zkp_fr_lincomb_dev(zkp_ctx* ctx, zkp_curve_t curve, size_t count, const uint64_t* const* p_dev, const size_t* ns,
                           const uint64_t* coeffs_host, uint64_t* out_dev, size_t n_out);
/* KZG10::commit / open (marlin/src/pc/kzg10.rs:108-109,137-140): MSM of Montgomery Fr coefficients that are already
 * on the DEVICE against powers[offset ..] (offset = number of skipped leading zeros) */
int32_t zkp_msm_g1_mont_dev(zkp_ctx* ctx, uint64_t handle, size_t offset, const uint64_t* fr_scalars_dev, size_t n,
                            uint64_t* out_xyz_host);
int32_t zkp_msm_g2_mont_dev(zkp_ctx* ctx, uint64_t handle, size_t offset, const uint64_t* fr_scalars_dev, size_t n,
                            uint64_t* out_xyz_host);
/* PC::commit over a LIST of polynomials (marlin/src/pc/mod.rs:34-71; one KZG10::commit = one MSM each, kzg10.rs:100-123):
 * `count` MSMs of device-resident Montgomery coefficient vectors against powers[offsets[k] ..], min(ns[k], len - offset)
 * terms each, three in flight at a time on the context's MSM streams.  out_xyz: count Jacobian results. */
int32_t zkp_msm_g1_mont_batch_dev(zkp_ctx* ctx, uint64_t bases_handle, size_t count, const size_t* offsets,
                                  const uint64_t* const* scalars_dev, const size_t* ns, uint64_t* out_xyz);
/* The same for MSMs against DIFFERENT resident base vectors (G1 and G2 mixed): the five partial MSMs of a base-sharded
 * Groth16 proof (prover.rs:164-190) in one call, four in flight.  Result k is written at out_xyz + k * slot_u64 (its
 * Jacobian limbs first); slot_u64 >= 3 * limbs of the largest group involved (18 for BN254 G2, 36 for BLS12-381 G2). */
int32_t zkp_msm_mont_multi_dev(zkp_ctx* ctx, size_t count, const uint64_t* bases_handles, const size_t* offsets,
                               const uint64_t* const* scalars_dev, const size_t* ns, uint64_t* out_xyz, size_t slot_u64);
/* fold k Jacobian points (host) into one: the local step after the multi-GPU all-gather of partial MSM
 * results (EC addition is not an RCCL reduction op) */
int32_t zkp_g1_fold(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xyz_host, size_t k, uint64_t* out_xyz);
int32_t zkp_g2_fold(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xyz_host, size_t k, uint64_t* out_xyz);
/* Jacobian -> affine (x, y) + identity flag: ark `into_affine()` */
int32_t zkp_g1_into_affine(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xyz_host, uint64_t* xy_out,
                           uint8_t* inf_out);
int32_t zkp_g2_into_affine(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xyz_host, uint64_t* xy_out,
                           uint8_t* inf_out);
/* HOST ONLY (no device, ctx may be NULL-free: there is none): the into_affine() of the three proof points (prover.rs:205-209) as
 * zkp_groth16_prove* runs it since ABI 0.4 — a, c: G1 XYZZ (x = X / ZZ, y = Y / ZZZ; ZZ == 0: the identity; 4 coordinates of
 * L u64 limbs, Montgomery), b: G2 XYZZ (8 coordinates, (c0, c1) pairs) -> proof_out = A | B | C affine Montgomery words exactly as
 * zkp_groth16_prove writes them (ark's (0, 0) for the identity), inf_out[3].  One field inversion for all three points. */
int32_t zkp_groth16_points_into_affine(zkp_curve_t curve, const uint64_t* a_xyzz, const uint64_t* b_xyzz, const uint64_t* c_xyzz,
                                       uint64_t* proof_out, uint8_t* inf_out);

/* ark-serialize 0.2 COMPRESSED short-Weierstrass points <-> the affine Montgomery arrays of zkp_groth16_pk_desc /
 * zkp_bases_upload_*: what `Parameters::serialize` writes into a .pk file (cli/src/setup.rs:41-45) and `Proof::serialize` into
 * a proof (cli/src/zkp_prove.rs:45-49).  A point is its canonical little-endian x (G2: c0 then c1; 32 / 64 bytes on BN254,
 * 48 / 96 on BLS12-381) with two flags in the top bits of the last byte: bit 7 = y is the larger of {y, -y} (Fq: as integers;
 * Fq2: c1 first, then c0), bit 6 = the identity.  Decompression (a square root per point) runs on the device, one lane per point:
 * a 2^20 key loads in tens of milliseconds.  On a malformed point (both flags, x >= p, x^3 + b not a square) the call returns
 * ZKP_ERR_INVALID_POINT, *bad_index (if not NULL) receives its index and xy_out / inf_out are left untouched (*bad_index is
 * SIZE_MAX after any other outcome, so an argument error is never mistaken for "point 0").  No subgroup check (= ark's `deserialize_unchecked` for the
 * cofactor groups; BN254 G1 has cofactor 1).  The container framing (Vec length prefixes, field order of `Parameters`) stays with
 * the caller: ckb_zkp_amd/serialize.py, rust/zkp-accel. */
int32_t zkp_g1_decompress(zkp_ctx* ctx, zkp_curve_t curve, const uint8_t* bytes, size_t n, uint64_t* xy_out, uint8_t* inf_out,
                          size_t* bad_index);
int32_t zkp_g2_decompress(zkp_ctx* ctx, zkp_curve_t curve, const uint8_t* bytes, size_t n, uint64_t* xy_out, uint8_t* inf_out,
                          size_t* bad_index);
int32_t zkp_g1_compress(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* bytes_out);
int32_t zkp_g2_compress(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* bytes_out);
/* The CHECKED half of ark-serialize's `deserialize` for curve points (ark-ec 0.2 `GroupAffine::deserialize`: on the curve and
 * `is_in_correct_subgroup_assuming_on_curve`, i.e. [r]P = O; what `Parameters::deserialize` / `Proof::deserialize` /
 * `VerifyKey::deserialize` run per element — /root/reference/cli/src/zkp_prove.rs:45, zkp_verify.rs:61-62).  xy: n affine Montgomery points
 * (the layout zkp_g*_decompress writes), inf: optional identity flags (identities pass).  One lane per point, a double-and-add over
 * the group order: ~0.2 s for a 2^20-element G2 query.  ZKP_OK if every point passes; otherwise ZKP_ERR_INVALID_POINT and *bad_index
 * (if not NULL) = index of the first point that is off the curve or outside the prime-order subgroup. */
int32_t zkp_g1_subgroup_check(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n, size_t* bad_index);
int32_t zkp_g2_subgroup_check(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* xy, const uint8_t* inf, size_t n, size_t* bad_index);

/* ---- fixed-base multiples k_i * P (setup side, generator.rs:205-256 `FixedBaseMSM`).
 * Used to build synthetic proving keys from a known trapdoor at 2^20+ scale.  scalars canonical. */
int32_t zkp_fixed_base_mul_g1(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* base_xy, const uint64_t* scalars_host,
                              size_t n, uint64_t* out_xy, uint8_t* out_inf);
int32_t zkp_fixed_base_mul_g2(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* base_xy, const uint64_t* scalars_host,
                              size_t n, uint64_t* out_xy, uint8_t* out_inf);

/* ---- Groth16: replaces zkp_groth16::create_proof (groth16/src/prover.rs:124-211) ---------------
 * The circuit closures stay on the caller's side (Rust); the boundary receives what
 * `ProvingAssignment` holds after synthesis (prover.rs:16-25): the three sparse matrices and the
 * assignment.  Matrices are fixed per circuit -> uploaded with the key.
 * A descriptor with a_query == NULL uploads the matrices only (witness_map works, prove is refused): used by
 * the base-sharded multi-GPU prover, where every rank holds the matrices and a slice of each query. */
typedef struct {
  /* CSR over constraints; coeffs Fr Montgomery; col = index into z = input_assignment ++ aux_assignment */
  const uint32_t* row_ptr; /* num_constraints + 1 */
  const uint32_t* col;     /* nnz */
  const uint64_t* coeff;   /* nnz x 4 */
} zkp_csr;

typedef struct {
  zkp_curve_t curve;
  uint32_t num_inputs;      /* incl. the constant one */
  uint32_t num_aux;
  uint32_t num_constraints;
  zkp_csr at, bt, ct;       /* prover.rs:17-19 */
  /* Parameters<E> (groth16/src/lib.rs:79-91), host affine Montgomery + identity flags (NULL = none) */
  const uint64_t* alpha_g1; const uint64_t* beta_g1; const uint64_t* delta_g1; /* 1 G1 point each */
  const uint64_t* beta_g2; const uint64_t* delta_g2;                           /* 1 G2 point each */
  const uint64_t* a_query; const uint8_t* a_inf; size_t a_len;
  const uint64_t* b_g1_query; const uint8_t* b_g1_inf; size_t b_g1_len;
  const uint64_t* b_g2_query; const uint8_t* b_g2_inf; size_t b_g2_len;
  const uint64_t* h_query; const uint8_t* h_inf; size_t h_len;
  const uint64_t* l_query; const uint8_t* l_inf; size_t l_len;
} zkp_groth16_pk_desc;

typedef struct zkp_groth16_pk zkp_groth16_pk; /* opaque device-resident proving key */

/* Uploads `Parameters<E>` + the circuit matrices once; every zkp_groth16_prove* call then runs on the resident key.  Besides the
 * window tables the upload derives (round 4, one-time, on the device: + 0.65 s at 2^20, linear in N log N; sharded keys likewise):
 *   - the h_query in EVALUATION form over the coset of r1cs_to_qap.rs:164-169, so that the H MSM of prover.rs:186-187 takes the
 *     pointwise values (a b - c) / Z(g) and the closing coset_ifft is not run;
 *   - the l_query with the C matrix folded in (L'_m = L_m - sum_k C_km G_k), so that neither C z nor the ifft / coset_fft of c
 *     (r1cs_to_qap.rs:155-162) is run.
 * Proofs are the group elements of prover.rs:192-210 for every assignment, satisfying or not; zkp_groth16_witness_map still
 * returns h in coefficient form.  ZKP_H_LAGRANGE=0 / ZKP_C_FOLD=0 keep the key as given (21 instead of 12 transform passes). */
int32_t zkp_groth16_pk_upload(zkp_ctx* ctx, const zkp_groth16_pk_desc* desc, zkp_groth16_pk** out);
/* The same with flags (ABI 0.5).  ZKP_PK_KEEP_FORM: skip the evaluation-form transforms above — the key stays as `Parameters<E>` holds it
 * (upload ~0.65 s shorter per 2^20 constraints, a proof runs all 7 transforms of r1cs_to_qap.rs:144-169: 7.0 instead of 6.5 ms at 2^20).
 * For callers that prove once or a few times per key, e.g. the reference CLI (cli/src/zkp_prove.rs loads a key, proves, exits): the
 * transforms pay back after ~2000 proofs.  Same proof bytes either way.  Unknown flag bits -> ZKP_ERR_BAD_ARG. */
#define ZKP_PK_KEEP_FORM 1u
int32_t zkp_groth16_pk_upload_ex(zkp_ctx* ctx, const zkp_groth16_pk_desc* desc, uint32_t flags, zkp_groth16_pk** out);
int32_t zkp_groth16_pk_free(zkp_ctx* ctx, zkp_groth16_pk* pk);

/* R1CStoQAP::witness_map (groth16/src/r1cs_to_qap.rs:113-172): z (num_inputs+num_aux Fr, Montgomery)
 * -> h (domain_size Fr, Montgomery).  *_dev: both pointers are device memory. */
int32_t zkp_groth16_witness_map(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint64_t* z_host, uint64_t* h_host);
int32_t zkp_groth16_witness_map_dev(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint64_t* z_dev, uint64_t* h_dev);
int32_t zkp_groth16_domain_size(zkp_groth16_pk* pk, uint64_t* n);
/* Window-table plan of a resident key: info[0] = window-group size k (1 = one table copy per window; > 1: the tables did not
 * fit ZKP_TABLE_BUDGET_GB / the free device memory and k consecutive windows share a copy), info[1] = bytes of the five
 * queries' tables, info[2..4] = window bits / windows / resident copies of the A query, info[5] = window bits of the B queries,
 * info[6] = sort sharing (bit 0: B1 reuses B2's bucket sort, bit 1: L reuses A's, bit 2: shared level-1 pass; bits 32..63: how many
 * fused proof groups the pipelined batches of this key have run so far, warm-up groups left out), info[7] = key form (bit 0: H query in evaluation form, bit 1: C folded into the L query, bit 2: L and H
 * bucket-chained).  With any bit of info[7] set, slots L (3) and H (4) of zkp_groth16_prove_partials_dev are NOT the reference's
 * l_aux_acc / h_acc individually — only slot 3 + slot 4 equals l_aux_acc + h_acc, which is all prover.rs:189-196 consumes
 * (ZKP_H_LAGRANGE=0 ZKP_C_FOLD=0 ZKP_CHAIN_LH=0 at upload restores the individual values). */
int32_t zkp_groth16_pk_info(zkp_ctx* ctx, zkp_groth16_pk* pk, uint64_t info[8]);

/* create_proof(params, circuit, r, s): z = full assignment (Montgomery), r/s Fr Montgomery (4 limbs).
 * proof_out: A (G1 affine) | B (G2 affine) | C (G1 affine), Montgomery; inf_out[3] identity flags. */
int32_t zkp_groth16_prove(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint64_t* z_host, const uint64_t* r,
                          const uint64_t* s, uint64_t* proof_out, uint8_t* inf_out);
int32_t zkp_groth16_prove_dev(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint64_t* z_dev, const uint64_t* r,
                              const uint64_t* s, uint64_t* proof_out, uint8_t* inf_out);

/* Throughput mode: n independent proofs with the same key, software-pipelined inside the library over two
 * "lanes" (stream sets + scratch), so that the latency-bound tail of proof i (log-depth bucket reduction, the two
 * dynamic scalar multiplications of the assembly) overlaps the throughput-bound kernels of proof i+1.
 * z_dev: n device pointers (may repeat); r, s: n x 4 limbs (host); proofs_out: n x (A|B|C); inf_out: n x 3. */
int32_t zkp_groth16_prove_batch_dev(zkp_ctx* ctx, zkp_groth16_pk* pk, size_t n, const uint64_t* const* z_dev,
                                    const uint64_t* r, const uint64_t* s, uint64_t* proofs_out, uint8_t* inf_out);

/* The same with the witnesses in HOST memory: each proof's assignment (num_inputs + num_aux Fr) is copied to the device on
 * its lane's stream in front of the proof, so the PCIe transfer of proof i+1 overlaps the kernels of proof i when the
 * host buffers are pinned (hipHostMalloc / hipHostRegister); pageable buffers work but the copy then blocks the caller. */
int32_t zkp_groth16_prove_batch(zkp_ctx* ctx, zkp_groth16_pk* pk, size_t n, const uint64_t* const* z_host,
                                const uint64_t* r, const uint64_t* s, uint64_t* proofs_out, uint8_t* inf_out);

/* Multi-GPU (one process per GPU, bases sharded by index): every rank computes partial sums with zkp_msm_*,
 * the host all-gathers them (RCCL / any transport: 5 points, < 2 KiB), folds them with zkp_g*_fold and finishes
 * here.  sums_xyz: Jacobian Montgomery  g_a (G1) | g1_b (G1) | g2_b (G2) | h_acc (G1) | l_acc (G1)  where the
 * key-point terms of prover.rs:165-177,183 are already folded in (see DESIGN.md "Folding").  Computes
 * C = s*g_a + r*g1_b + l_acc + h_acc and the three into_affine() (prover.rs:192-210). */
int32_t zkp_groth16_assemble(zkp_ctx* ctx, zkp_curve_t curve, const uint64_t* sums_xyz, const uint64_t* r,
                             const uint64_t* s, uint64_t* proof_out, uint8_t* inf_out);

/* Device-resident base-sharded step (BASELINE configs[4]) — nothing but the collective between the calls:
 *   zkp_groth16_pk_upload_shard     rank `rank` of `world` keeps elements [lo, hi) of every query of prover.rs:164-190
 *                                   resident (contiguous, balanced ranges over the extended queries; 1/world of the key)
 *                                   plus the circuit matrices;
 *   zkp_groth16_prove_partials_dev  witness map (replicated) + the five partial MSMs of this rank; r, s (host, Montgomery)
 *                                   must be the same on every rank.  partials_dev (DEVICE, zkp_groth16_partials_bytes()
 *                                   bytes: 5 XYZZ slots A|B1|B2|H|L) is complete when the call returns; only the slot-wise
 *                                   SUMS over the ranks are specified — since round 3 the H MSM reduces L's buckets
 *                                   together with its own (slot H = h_acc + l', slot L = the identity; C uses their sum);
 *   -- ncclAllGather(partials_dev -> gathered_dev, world x partials bytes) over RCCL, by the caller --
 *   zkp_groth16_fold_assemble_dev   slot-wise sum over the ranks (EC addition is not an RCCL reduction op) + assembly of
 *                                   prover.rs:192-210 -> proof_out (host).
 * A sharded key is refused by zkp_groth16_prove*. */
int32_t zkp_groth16_pk_upload_shard(zkp_ctx* ctx, const zkp_groth16_pk_desc* desc, int32_t rank, int32_t world,
                                    zkp_groth16_pk** out);
int32_t zkp_groth16_partials_bytes(zkp_curve_t curve, size_t* bytes);
int32_t zkp_groth16_prove_partials_dev(zkp_ctx* ctx, zkp_groth16_pk* pk, const uint64_t* z_dev, const uint64_t* r,
                                       const uint64_t* s, void* partials_dev);
int32_t zkp_groth16_fold_assemble_dev(zkp_ctx* ctx, zkp_curve_t curve, const void* gathered_dev, int32_t world,
                                      const uint64_t* r, const uint64_t* s, uint64_t* proof_out, uint8_t* inf_out);

/* ---- Single-process multi-GPU: `create_proof` (groth16/src/prover.rs:124) is ONE call in ONE process, so the library owns
 * one context per device and the exchange step (zkp_ctx_create(ctx**, device_ids, n_devices)).
 *   zkp_ctx_create_multi   root context = rank 0 (device_ids[0]) + one member context per further id, rank order = argument
 *                          order.  Ids may repeat (several ranks on one GPU: one-GPU test boxes).  Peer access between
 *                          distinct devices is enabled when the topology offers it (xGMI).  The root is an ordinary
 *                          zkp_ctx for every other call; zkp_ctx_destroy(root) destroys the members.
 *   zkp_ctx_device         borrow member `rank` (rank 0 = the root itself) for zkp_dev_alloc / zkp_h2d / ... on that device.
 *   zkp_groth16_pk_upload_multi
 *       ZKP_MULTI_SHARD      every (extended) query of prover.rs:164-190 split by index, rank k keeps 1/n of the window
 *                            tables (BASELINE configs[4]: keys that do not fit one GPU; lower single-proof latency);
 *       ZKP_MULTI_REPLICATE  the whole key on every device (throughput: independent proofs on independent GPUs).
 *   zkp_groth16_prove_multi        (SHARD key) ONE proof over all devices: partial MSMs per device, the five partial sums
 *                          exchanged over xGMI — an RCCL ncclAllGather of n x zkp_groth16_partials_bytes whenever the
 *                          devices are distinct and librccl.so loads (dlopen, no link-time dependency), else
 *                          hipMemcpyPeerAsync to rank 0, said once on stderr (ZKP_MULTI_EXCHANGE=rccl / peer forces one) —
 *                          then slot-wise fold + assembly on rank 0.  With n >= 3 the witness map can be task-split: the
 *                          a / b / c chains of r1cs_to_qap.rs:144-162 on ranks 0 / 1 / 2, rank 0 finishes h and every rank
 *                          fetches its slice of h for its share of the H MSM.  Whether that beats the replicated map depends
 *                          on the link, so the key measures both on its own proofs 3 and 4 (1 and 2 warm them up) and keeps
 *                          the faster from proof 5 on; the proof bytes do not depend on it (ZKP_MULTI_WM_SPLIT=0 / 1
 *                          forces).  z_on_device == 0: z[0] is the host assignment; != 0: z[k] is a device pointer on rank
 *                          k's device, k < n.
 *   zkp_groth16_multi_info  what the last zkp_groth16_prove_multi did: info[0] = exchange (0 peer copies, 1 RCCL all-gather, 2 peer copies because
 *                          the RCCL watchdog gave up: ncclCommInitAll or the probe all-gather failed or did not return within
 *                          zkp_ctx_config.multi_exchange_timeout_ms — RCCL then stays off for the process),
 *                          info[1] = RCCL ranks, info[2] = witness map (0 replicated, 1 split, 2 still measuring), info[3] /
 *                          info[4] = microseconds of the timed proof with the replicated / split map (0 = not measured),
 *                          info[5] = devices.
 *   zkp_groth16_prove_batch_multi  (REPLICATE key) `count` independent proofs, proof i on rank i % n (z[i] host, or a device
 *                          pointer on that rank's device), one host thread per device driving its lanes as
 *                          zkp_groth16_prove_batch does; outputs in input order. */
typedef struct zkp_groth16_pk_multi zkp_groth16_pk_multi;
typedef enum { ZKP_MULTI_SHARD = 0, ZKP_MULTI_REPLICATE = 1 } zkp_multi_mode;
int32_t zkp_ctx_create_multi(zkp_ctx** out, const int* device_ids, int n_devices);
/* the same with a configuration applied to the root and every member (cfg == NULL: defaults) */
int32_t zkp_ctx_create_multi_ex(zkp_ctx** out, const int* device_ids, int n_devices, const zkp_ctx_config* cfg);
int32_t zkp_ctx_num_devices(zkp_ctx* ctx, int32_t* n);
int32_t zkp_ctx_device(zkp_ctx* ctx, int32_t rank, zkp_ctx** member);
int32_t zkp_groth16_pk_upload_multi(zkp_ctx* ctx, const zkp_groth16_pk_desc* desc, int32_t mode,
                                    zkp_groth16_pk_multi** out);
int32_t zkp_groth16_pk_multi_free(zkp_ctx* ctx, zkp_groth16_pk_multi* pk);
int32_t zkp_groth16_multi_info(zkp_ctx* ctx, zkp_groth16_pk_multi* pk, uint64_t info[6]);
int32_t zkp_groth16_prove_multi(zkp_ctx* ctx, zkp_groth16_pk_multi* pk, const uint64_t* const* z, int32_t z_on_device,
                                const uint64_t* r, const uint64_t* s, uint64_t* proof_out, uint8_t* inf_out);
int32_t zkp_groth16_prove_batch_multi(zkp_ctx* ctx, zkp_groth16_pk_multi* pk, size_t count, const uint64_t* const* z,
                                      int32_t z_on_device, const uint64_t* r, const uint64_t* s, uint64_t* proofs_out,
                                      uint8_t* inf_out);

/* ---- Marlin Fiat–Shamir RNG (host code): replaces marlin/src/fs_rng.rs:11-70 `FiatShamirRng` ----------------------------
 * merlin 2.0 transcript "MARLINSEED" -> 32-byte seed -> ChaCha20 RNG (rand_chacha 0.2).  The byte strings absorbed are
 * the caller's `to_bytes![...]` (marlin/src/lib.rs:105-158); samples come back in the ABI's field layout.
 *   new                  FiatShamirRng::from_seed(&bytes)                       fs_rng.rs:41-53
 *   absorb               seed = H(bytes || seed), re-key the ChaCha stream      fs_rng.rs:57-69
 *   rand_fr              `Fr::rand(&mut fs_rng)` (ark-ff 0.2 rejection sampling; Montgomery limbs out)
 *   sample_outside_domain  AHP::sample_element_outside_domain for a domain of 2^log_domain (ahp/verifier.rs:118-127)
 *   rand_u128            `u128::rand(&mut fs_rng)` -> out[0] = low, out[1] = high 64 bits (lib.rs:158)
 *   seed / next_u64      introspection for the parity tests
 *   zkp_merlin_oneshot   Transcript::new(label); append_message(msg_label, msg); challenge_bytes(chal_label, out) */
typedef struct zkp_fs_rng zkp_fs_rng;
int32_t zkp_fs_rng_new(const uint8_t* seed_material, size_t len, zkp_fs_rng** out);
int32_t zkp_fs_rng_free(zkp_fs_rng* rng);
int32_t zkp_fs_rng_absorb(zkp_fs_rng* rng, const uint8_t* material, size_t len);
int32_t zkp_fs_rng_seed(const zkp_fs_rng* rng, uint8_t out32[32]);
int32_t zkp_fs_rng_next_u64(zkp_fs_rng* rng, uint64_t* out);
int32_t zkp_fs_rng_rand_u128(zkp_fs_rng* rng, uint64_t out[2]);
int32_t zkp_fs_rng_rand_fr(zkp_fs_rng* rng, zkp_curve_t curve, uint64_t* out_mont);
int32_t zkp_fs_rng_sample_outside_domain(zkp_fs_rng* rng, zkp_curve_t curve, uint32_t log_domain, uint64_t* out_mont);
int32_t zkp_merlin_oneshot(const uint8_t* label, size_t label_len, const uint8_t* msg_label, size_t msg_label_len,
                           const uint8_t* msg, size_t msg_len, const uint8_t* chal_label, size_t chal_label_len,
                           uint8_t* out, size_t out_len);

/* ---- Marlin: replaces zkp_marlin::index (device half) and zkp_marlin::create_random_proof (marlin/src/lib.rs:69-181) ----
 * The caller keeps synthesis and the index-manipulation half of AHP::index (make_matrices_square, balance_matrices, per-row
 * column sort: ahp/constraint_systems.rs:9-31,100-133) and hands over the three square matrices as CSR; the library computes
 * the arithmetization (row / col / val / row_col over K, their interpolations and evaluations over B: arithmetic.rs:98-172)
 * on the device and keeps it resident.  `zkp_marlin_prove` runs prover_init and the three AHP rounds (ahp/prover.rs:86-427),
 * PC::commit after each round (pc/mod.rs:34-71, MSMs on the resident SRS powers), the Fiat–Shamir transcript
 * (fs_rng.rs; lib.rs:105-158), the 21 evaluations and PC::batch_open (pc/mod.rs:73-160).  The zk randomness the reference
 * draws from `zk_rng` (mask polynomial, the three degree-0 masks, the hiding-bound-1 commitment blinders) is an input. */
typedef struct zkp_marlin_index zkp_marlin_index;
typedef struct {
  zkp_curve_t curve;
  uint32_t num_inputs; /* formatted public inputs incl. the leading one */
  uint32_t n;          /* rows == columns after make_matrices_square */
  uint32_t pad_aux;    /* dummy witness variables (value one) make_matrices_square appended */
  zkp_csr a, b, c;     /* n rows each, balanced, columns ascending per row, col < n; coeffs Fr Montgomery */
} zkp_marlin_index_desc;
#define ZKP_MARLIN_NUM_EVALS 21
typedef struct {
  const uint64_t* w;   /* 1 Fr (Montgomery) each: the degree-0 masks of prover.rs:190,196,200 */
  const uint64_t* z_a;
  const uint64_t* z_b;
  const uint64_t* mask;    /* 3|H| Fr: DensePolynomial::rand of prover.rs:202-203 (host, or device if mask_on_device) */
  int32_t mask_on_device;
  const uint64_t* blind_w; /* 2 Fr each: `Rand::rand(hiding_bound = 1)` of KZG10::commit for w, z_a, z_b, g_1 and g_1's shifted commitment */
  const uint64_t* blind_z_a;
  const uint64_t* blind_z_b;
  const uint64_t* blind_g_1;
  const uint64_t* blind_shifted_g_1;
} zkp_marlin_rand;
typedef struct {
  /* commitments in oracle order w, z_a, z_b, mask | t, g_1, h_1 | g_2, h_2: G1 affine Montgomery in 12-u64 slots */
  uint64_t comm[9 * 12];
  uint8_t comm_inf[9];
  uint64_t shifted[2 * 12]; /* degree-bound commitments of g_1 and g_2 */
  uint8_t shifted_inf[2];
  uint64_t evaluations[ZKP_MARLIN_NUM_EVALS * 4]; /* query-set order = labels ascending (lib.rs:147-156), Fr Montgomery */
  uint32_t num_opening_proofs;                    /* 2 (1 if beta == gamma); query points ascending */
  uint64_t opening_w[2 * 12];
  uint8_t opening_w_inf[2];
  uint8_t opening_has_rand[2];
  uint64_t opening_rand_v[2 * 4];
  uint64_t challenges[7 * 4]; /* alpha, eta_a, eta_b, eta_c, beta, gamma, opening challenge (Fr Montgomery) as used */
} zkp_marlin_proof;
int32_t zkp_marlin_index_upload(zkp_ctx* ctx, const zkp_marlin_index_desc* desc, zkp_marlin_index** out);
int32_t zkp_marlin_index_free(zkp_ctx* ctx, zkp_marlin_index* index);
/* info[6] = |X|, |H|, |K|, |B|, max_degree (= the SRS degree `index.max_degree()` needs), num_non_zeros */
int32_t zkp_marlin_index_info(const zkp_marlin_index* index, uint64_t info[6]);
/* the 12 index commitments (lib.rs:77-83; a_row, a_col, a_val, a_row_col, b_..., c_...): G1 affine Montgomery, 12-u64 slots */
int32_t zkp_marlin_index_commit(zkp_ctx* ctx, zkp_marlin_index* index, uint64_t powers_of_g, uint64_t* comms_xy,
                                uint8_t* inf);
/* powers_of_g / powers_of_gamma_g: resident bases (zkp_bases_upload_g1) of the committer key, >= max_degree + 1 / >= 2 points.
 * ivk_bytes = to_bytes![index_verifier_key] (the caller owns and serialises the key); x: num_inputs formatted inputs
 * (leading one included), w: the witness without the make_matrices_square padding — Fr Montgomery, host.
 * fixed_challenges == NULL: create_random_proof (messages derived from the transcript).  Non-NULL (7 Fr Montgomery: alpha,
 * eta_a, eta_b, eta_c, beta, gamma, xi): TEST HOOK — the messages are taken as given, the transcript is not consulted.
 * An index owns the scratch pool and the pinned landing slots of its proofs: ONE zkp_marlin_prove at a time per index (prove
 * with the same circuit from several threads = one zkp_marlin_index_upload per thread).  On any error the call drains its
 * streams before the pool is recycled, so a failed proof never leaves work in flight on the index. */
int32_t zkp_marlin_prove(zkp_ctx* ctx, zkp_marlin_index* index, uint64_t powers_of_g, uint64_t powers_of_gamma_g,
                         const uint8_t* ivk_bytes, size_t ivk_len, const uint64_t* x, const uint64_t* w, size_t n_w,
                         const zkp_marlin_rand* rnd, const uint64_t* fixed_challenges, zkp_marlin_proof* out);

/* ---- introspection for bench.py / rocprof bookkeeping ------------------------------------------ */
typedef struct {
  float ms_total;          /* last zkp_groth16_prove*: stream time, HIP events */
  float ms_witness_map;
  float ms_msm[5];         /* A, B1, B2, H, L */
  float ms_assemble;
  float ms_msm_accumulate; /* sum over the five MSMs of the bucket-accumulate kernel (dominant kernel) */
  uint64_t msm_accumulate_launches;
  uint64_t msm_points;     /* (scalar, window) entries of the five MSMs = mixed additions of the accumulate kernels */
  float ms_msm_scan;       /* MSM "scalar scan" (digit extraction fused into the level-1 histogram + scatter passes), summed */
  uint64_t msm_scan_launches; /* MSMs that ran their own scan (B1 reuses B2's) */
  uint64_t msm_scan_bytes; /* algorithmic bytes of those scans: 2 x 32 B per scalar read + 8 B per entry written */
  float ms_msm_acc[5];     /* accumulate kernel per MSM (A, B1, B2, H, L) */
  uint64_t msm_entries[5]; /* entries (= mixed additions: identity bases and zero digits are dropped by the scan) per MSM */
} zkp_groth16_timing;
int32_t zkp_groth16_last_timing(zkp_ctx* ctx, zkp_groth16_timing* out);
/* Phases of the last zkp_marlin_prove on this context (host clock around stream synchronisations that the prover performs
 * anyway between a round and its PC::commit, marlin/src/lib.rs:105-181): rounds = AHP prover rounds (sparse products, NTTs,
 * pointwise work), commits = the batched commitment MSMs of the round + the transcript, evaluations = 21 Horner evaluations,
 * open = batch_open (linear combinations, two witness divisions, two opening MSMs). */
typedef struct {
  double ms_round[3];
  double ms_commit[3];
  double ms_evaluations;
  double ms_open;
  double ms_total;
  uint64_t commit_points;  /* sum of the lengths of the committed coefficient vectors (incl. shifted commitments) */
  uint64_t open_points;    /* lengths of the opening-witness MSMs */
  uint64_t ntt_count;      /* transforms run by the three rounds */
  uint64_t ntt_elements;   /* sum of their sizes */
} zkp_marlin_timing;
int32_t zkp_marlin_last_timing(zkp_ctx* ctx, zkp_marlin_timing* out);
int32_t zkp_set_profiling(zkp_ctx* ctx, int32_t enable); /* per-phase HIP events (adds sync points) */
/* Sustained rate (1e9 products / s) of the library's own Montgomery multipliers with every CU saturated: the integer-VALU
 * roof the MSM / NTT kernels are bound by, measured in the calling process (bench.py `valu_roof`).
 * field: 0 = Fr, 1 = Fq; unsaturated: 0 = 32-bit saturated limbs (field_dev.hpp), 1 = 29/28-bit limbs (unsat_dev.hpp). */
int32_t zkp_bench_mulmod(zkp_ctx* ctx, zkp_curve_t curve, int32_t field, int32_t unsaturated, double* gmulmod_per_s);
/* HBM bandwidth (GB/s, bytes read + bytes written) a plain streaming copy kernel reaches on this device between two freshly
 * allocated `bytes`-byte buffers (>= 1 MiB; use >= 1 GiB so that the 256 MB of Infinity Cache cannot hold it): the measured
 * peak bench.py quotes next to the nominal 8 TB/s ("also measure an on-box copy kernel and quote both"). */
int32_t zkp_bench_hbm_copy(zkp_ctx* ctx, size_t bytes, double* gbytes_per_s);

#ifdef __cplusplus
}
#endif
#endif /* ZKP_ACCEL_H */
