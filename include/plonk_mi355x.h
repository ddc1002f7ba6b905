/*
 * plonk_mi355x.h -- C ABI of the MI355X (gfx950) backend for the PLONK prover hot path:
 * BLS12-381 Fr radix-2 NTT / iNTT / coset-NTT and G1 variable-base MSM (KZG commit).
 *
 * Drop-in boundary.  The reference (Manta-Network/Plonk-Prototype) reaches this path only
 * through its dependencies (ref:Cargo.toml:19 `dusk-plonk = 0.8.2`, ref:Cargo.toml:20
 * `dusk-bls12_381 = 0.8`): there is no FFI or plugin interface upstream, `best_fft` and
 * `msm_variable_base` are plain Rust functions.  The entry points below are therefore
 * exactly what a `-sys` crate for a `[patch.crates-io]` fork of those two crates binds
 * (INTEGRATION.md shows the Rust side):
 *
 *   pm_fr_ntt / pm_fr_ntt_batch  <- dusk_plonk::fft::EvaluationDomain::{fft, ifft, coset_fft,
 *                                   coset_ifft}(_in_place)   [ark-poly: EvaluationDomain::
 *                                   {fft, ifft, coset_fft, coset_ifft}]   SURVEY.md 8a a3-a7
 *   pm_domain_info               <- EvaluationDomain::new  (group_gen, group_gen_inv,
 *                                   size_inv; error when log2(size) >= 32)  SURVEY.md 8a a2
 *   pm_g1_bases_upload           <- CommitKey { powers_of_g }  (device-resident SRS)   a10
 *   pm_g1_msm                    <- dusk_bls12_381::multiscalar_mul::msm_variable_base
 *                                   [ark-ec: VariableBaseMSM::multi_scalar_mul]        a9
 *   pm_g1_fold / pm_g1_to_affine <- G1Projective `+` / G1Affine::from (multi-GPU fold)  a8
 *   pm_fr_*_dev, pm_plonk_*_dev  <- fft::{Polynomial, Evaluations}, proof_system::{permutation,
 *                                   quotient_poly, linearisation_poly} pointwise work   8f N1/N2
 *   pm_plonk_preprocess / _prove <- proof_system::{ProverKey, Prover::prove_with_preprocessed}:
 *                                   the whole five-round prover behind one call        8f N1-N3
 *   pm_g1_fixed_base_mul_dev     <- PublicParameters::setup (powers of tau)             8f N4
 *   pm_g1_bases_from_compressed  <- CommitKey::from_slice / PublicParameters::from_slice (checked SRS loading),
 *   pm_g1_decompress / _compress    G1Affine::{from_compressed, to_compressed}           8f N4
 *   pm_g1_scalar_mul_dev         <- `G1Affine * Scalar` in bulk (an SRS update: powers[i] * delta^i)
 * (include/plonk_mi355x.hpp is the C++ mirror of the same interfaces.)
 *
 * Data layouts are the Rust types' memory, so slices can be passed without marshalling:
 *   Fr  (BlsScalar / ark Fr)  : 4 x uint64_t little-endian limbs, Montgomery form R = 2^256,
 *                               fully reduced.  32 bytes, 8-byte aligned.
 *   Fp                        : 6 x uint64_t little-endian limbs, Montgomery form R = 2^384.
 *   G1 affine base            : x[6] | y[6]  (96 bytes packed).  The point at infinity is
 *                               encoded as x = y = 0 (not on the curve, so unambiguous).
 *   G1 projective result      : X[6] | Y[6] | Z[6] (144 bytes), always normalised to Z = 1
 *                               (Montgomery one) or (0, 1, 0) for the identity -- valid both
 *                               as dusk/zkcrypto homogeneous and as ark Jacobian coordinates.
 *
 * Ownership: the caller owns every host buffer; the library never keeps a host pointer past
 * return.  pm_ctx / pm_bases are library-owned handles freed by pm_shutdown / pm_g1_bases_free.
 * Errors: every call returns PM_OK (0) or a negative pm_status; nothing unwinds across the
 * ABI.  pm_last_error(ctx) gives a human-readable string for the last failure on that ctx.
 * Threading: calls on one ctx are serialised by an internal mutex; use one ctx per thread
 * for concurrency (a pm_prover_key carries its proof workspace: one proof at a time per key).  One ctx drives one GPU (one process per GPU under torch.distributed).
 * There is no CPU fallback: without a usable gfx950 device pm_init fails with
 * PM_ERR_NO_DEVICE.
 */
#ifndef PLONK_MI355X_H
#define PLONK_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pm_ctx pm_ctx;
typedef struct pm_bases pm_bases;

typedef enum {
  PM_OK = 0,
  PM_ERR_BAD_ARG = -1,
  PM_ERR_DOMAIN_TOO_LARGE = -2, /* log_n >= 32 = Fr two-adicity (EvaluationDomain::new fails) */
  PM_ERR_OOM = -3,
  PM_ERR_HIP = -4,
  PM_ERR_NO_DEVICE = -5,
  PM_ERR_LENGTH = -6,           /* in_len > 2^log_n, or n > number of uploaded bases */
  PM_ERR_EXCHANGE = -7,         /* a multi-GPU exchange (callback or RCCL) failed or a peer gave up */
  PM_ERR_BUSY = -8,             /* the prover key's workspace is in use by another proof */
  PM_ERR_POINT = -9             /* a point failed decoding or a requested check; see bad_index / bad_reason */
} pm_status;

/* pm_fr_ntt flags */
#define PM_NTT_FORWARD 0u
#define PM_NTT_INVERSE 1u /* use group_gen_inv and scale by size_inv (ifft) */
#define PM_NTT_COSET 2u   /* fft: pre-scale a[i] *= 7^i ; with INVERSE: post-scale a[i] *= 7^-i */
#define PM_NTT_TRANSPOSED 4u /* pm_fr_ntt_fourstep_dev only: block-transposed order between a forward and an inverse transform */

/* pm_g1_msm scalar_form */
#define PM_SCALAR_MONTGOMERY 0u /* dusk `&[BlsScalar]` memory */
#define PM_SCALAR_CANONICAL 1u  /* ark `&[BigInteger256]` memory (plain integers < r) */

const char* pm_version(void);

/* Create a context on HIP device `device_id` (stream, twiddle caches, workspaces). */
int pm_init(int device_id, pm_ctx** out);
void pm_shutdown(pm_ctx* ctx);
const char* pm_last_error(const pm_ctx* ctx);
/* Block until everything queued on the context's stream has finished. */
int pm_sync(pm_ctx* ctx);
/* The context's own HIP stream (a hipStream_t; what hip_stream = NULL means in the *_dev entry points): for callers that
 * order their own work after the library's, or record timing events around it.  Owned by the context. */
void* pm_ctx_stream(pm_ctx* ctx);
/* Give back what the context caches between calls -- pass buffers, MSM / polynomial workspaces, staging, twiddle tables --
 * after waiting for the device; everything is rebuilt or regrown on demand (a workspace only ever grows otherwise: after
 * one 2^30-point transform a context holds 77 GB of pass buffers).  pm_bases and pm_prover_key objects are untouched.
 * freed_bytes (may be NULL): device memory returned to the driver.  May be called at any time from any thread; while a
 * pm_fr_ntt_fourstep_dev call of another thread is between two of its exchange steps on this context (it keeps table
 * pointers across them) the call changes nothing and returns PM_ERR_BUSY. */
int pm_trim(pm_ctx* ctx, size_t* freed_bytes);

/* ---- EvaluationDomain ------------------------------------------------------------------ */

/* EvaluationDomain::new(2^log_n): writes group_gen, group_gen_inv, size_inv (Montgomery Fr).
 * Pure host arithmetic, needs no context.  PM_ERR_DOMAIN_TOO_LARGE when log_n >= 32. */
int pm_domain_info(uint32_t log_n, uint64_t group_gen[4], uint64_t group_gen_inv[4],
                   uint64_t size_inv[4]);

/* EvaluationDomain's small helpers (dusk-plonk 0.8.2 fft::domain, ref:Cargo.toml:19) -- what a patch
 * at the quotient_poly::compute / linearisation_poly level calls besides the transforms.  The plain forms are pure host
 * arithmetic on host buffers and need no context; the _dev forms fill a device vector of 2^log_n canonical Fr (Montgomery
 * limbs) with the library's kernels (pm_fr_powers_dev, pm_fr_vec_op_dev, pm_fr_batch_inverse_dev) and return when it is
 * complete.  PM_ERR_DOMAIN_TOO_LARGE when log_n >= 32.
 *   evaluate_vanishing_polynomial(tau)             = tau^size - 1
 *   compute_vanishing_poly_over_coset(poly_degree)   out[i] = (g w^i)^poly_degree - 1, g = GENERATOR = 7, w = group_gen;
 *                                                    upstream asserts size > poly_degree: PM_ERR_BAD_ARG otherwise
 *   evaluate_all_lagrange_coefficients(tau)          out[i] = L_i(tau) = (tau^size - 1) / size * w^i / (tau - w^i);
 *                                                    tau = w^j in the domain: the indicator vector of j */
int pm_domain_evaluate_vanishing_polynomial(uint32_t log_n, const uint64_t tau[4], uint64_t out[4]);
int pm_domain_vanishing_poly_over_coset(uint32_t log_n, uint64_t poly_degree, uint64_t* out);
int pm_domain_vanishing_poly_over_coset_dev(pm_ctx* ctx, uint32_t log_n, uint64_t poly_degree, void* d_out, void* hip_stream);
int pm_domain_evaluate_all_lagrange_coefficients(uint32_t log_n, const uint64_t tau[4], uint64_t* out);
int pm_domain_evaluate_all_lagrange_coefficients_dev(pm_ctx* ctx, uint32_t log_n, const uint64_t tau[4], void* d_out,
                                                     void* hip_stream);

/* Build (and cache on the device) the twiddle tables of the 2^log_n domain: every table that fft, ifft,
 * coset_fft and coset_ifft of that size read under the options in force, for any input length.  Optional: the
 * first transform of a size builds what it reads itself. */
int pm_domain_prepare(pm_ctx* ctx, uint32_t log_n);

/* out[0 .. 2^log_n) = transform of in[0 .. in_len) zero-padded to 2^log_n (the reference's
 * `resize(size, zero)`).  Natural order in and out, canonical Montgomery limbs.
 * in == out is allowed (the *_in_place forms).  Host pointers. */
int pm_fr_ntt(pm_ctx* ctx, const uint64_t* in, size_t in_len, uint64_t* out, uint32_t log_n,
              uint32_t flags);

/* `batch` independent transforms of the same size (a prover round issues 4-6 of them).
 * Vector b starts at in + 4*b*in_stride / out + 4*b*out_stride (strides in Fr elements). */
int pm_fr_ntt_batch(pm_ctx* ctx, const uint64_t* in, size_t in_len, size_t in_stride,
                    uint64_t* out, size_t out_stride, uint32_t log_n, uint32_t batch,
                    uint32_t flags);

/* Same transform on DEVICE-resident data (addresses on ctx's GPU), asynchronous on
 * `hip_stream` (a hipStream_t; NULL = the context's own stream).  d_in == d_out allowed. */
int pm_fr_ntt_dev(pm_ctx* ctx, const void* d_in, size_t in_len, size_t in_stride, void* d_out,
                  size_t out_stride, uint32_t log_n, uint32_t batch, uint32_t flags,
                  void* hip_stream);

/* One 2^log_n-point transform whose vector is block-distributed in natural order over `world` ranks (one
 * process and one context per GPU): rank r passes its N/world elements in d_inout
 * (DEVICE memory, transformed in place: the rank's block of x -> the same block of the result) and a scratch
 * buffer d_stage of 2 N/world elements (N/world when world == 1).  Four-step decomposition with three all-to-all
 * transposes; the sub-transforms are the library's own batched passes and the result equals pm_fr_ntt_dev's bit
 * for bit.  `exchange` performs the all-to-all of equal blocks (block p of d_send goes to rank p, block p of
 * d_recv comes from rank p; it is called with the library's stream idle and must return with the data in place;
 * non-zero = failure); NULL uses the context's RCCL communicator (pm_comm_init) on the context's stream.
 * world must be a power of two dividing both 2^(log_n / 2) and 2^(log_n - log_n / 2); 2 <= log_n <= 26.
 * Runs on the context's own stream.  Mirrors nothing upstream: dusk-plonk is single-device.
 * PM_NTT_TRANSPOSED saves the third all-to-all where the natural order is not needed (evaluations that are only
 * consumed pointwise, e.g. the quotient): a FORWARD transform then leaves X[k2 N1 + k1] at position k1 N2 + k2 of the
 * N1 x N2 row-major matrix (N1 = 2^(log_n / 2), rows block-distributed: rank r holds k1 in [r N1 / W, (r + 1) N1 / W)),
 * and an INVERSE transform takes exactly that layout and returns natural order. */
typedef int (*pm_alltoall_fn)(void* user, void* d_send, void* d_recv, size_t bytes_per_peer);
int pm_fr_ntt_fourstep_dev(pm_ctx* ctx, void* d_inout, void* d_stage, uint32_t log_n, uint32_t world,
                           uint32_t rank, uint32_t flags, pm_alltoall_fn exchange, void* user);
/* The same for `batch` vectors in ONE sequence of exchanges (a prover round transforms 4 - 20 polynomials of one size: the
 * all-to-all carries the batch's blocks together, so the number of exchange CALLS does not grow with the batch).
 * d_inout: batch x N/world elements, vector v's block at element v N/world; d_stage: 2 x batch x N/world elements
 * (1 x when world == 1).  d_halo (optional; forward + PM_NTT_TRANSPOSED only; NULL otherwise): batch x N2 elements, N2 =
 * 2^(log_n - log_n / 2): vector v's copy of the FIRST ROW OF THE NEXT RANK's part of the block-transposed result (row 0 for the
 * last rank), i.e. the values at index + 1 of this rank's last row -- what a consumer that reads X[k + 1] beside X[k] (the
 * quotient's z(w X) and next-row wires) needs from its neighbour; it travels inside the second all-to-all as one more column
 * per peer, no exchange of its own.  d_stage then holds 2 x batch x (N/world + N2) elements -- with world == 1:
 * batch x (N + N2): the halo row is packed there too.  The call cannot check the size of d_stage: the caller sizes it by this
 * rule (the library's own caller, csrc/prover_dist.hip.h, allocates 2 x 20 x (m + n2) elements once per key).  d_halo
 * doubles as the halo switch: a non-NULL d_halo on a call that is not forward + PM_NTT_TRANSPOSED is PM_ERR_BAD_ARG.
 * pm_fr_ntt_fourstep_dev is this call with batch = 1 and no halo. */
int pm_fr_ntt_fourstep_batch_dev(pm_ctx* ctx, void* d_inout, uint32_t batch, void* d_halo, void* d_stage, uint32_t log_n,
                                 uint32_t world, uint32_t rank, uint32_t flags, pm_alltoall_fn exchange, void* user);
/* Exchange counters of this context since the last reset: out[0] = all-to-all calls (one per transpose step with world > 1,
 * whichever transport carried it), out[1] = bytes this rank sent in them, out[2] = fixed-size message all-gathers of the
 * sharded / distributed prover, out[3] = transpose steps of the rank-split transforms whatever the world size (each is one
 * all-to-all call as soon as world > 1).  What a multi-GPU deployment pays per proof, countable on one GPU. */
int pm_comm_stats(pm_ctx* ctx, uint64_t out[4], int reset);

/* ---- KZG commit: G1 MSM ---------------------------------------------------------------- */

/* Upload n affine bases (CommitKey::powers_of_g) once; they stay resident in HBM.  A pm_bases is read-only after
 * pm_g1_bases_precompute and may be used by every context on its device at the same time (several proofs in flight over one
 * SRS); free it once, after the last call that uses it has returned. */
int pm_g1_bases_upload(pm_ctx* ctx, const uint64_t* xy, size_t n, pm_bases** out);
/* Optional, for a long-lived SRS: build the table of window multiples 2^(c w) * bases[i] in HBM
 * ((ceil(256/c) - 1) x 96 n extra bytes; about 8 MSMs of time, once).  Every later MSM on these
 * bases then needs one bucket set and no doublings: ~15 % faster.  window_bits 0 = default (log2 n, at most 20). */
int pm_g1_bases_precompute(pm_ctx* ctx, pm_bases* bases, uint32_t window_bits);
/* The same from affine points already in device memory (n x 96 bytes, the layout above). */
int pm_g1_bases_from_dev(pm_ctx* ctx, const void* d_xy, size_t n, pm_bases** out);
void pm_g1_bases_free(pm_ctx* ctx, pm_bases* bases);
size_t pm_g1_bases_len(const pm_bases* bases);

/* out = sum_{i<n} scalars[i] * bases[i]   (msm_variable_base(&bases[..n], scalars)).
 * Host scalars, n x 4 limbs.  n == 0 gives the identity. */
int pm_g1_msm(pm_ctx* ctx, const pm_bases* bases, size_t n, const uint64_t* scalars,
              uint32_t scalar_form, uint64_t out_xyz[18]);

/* Device-resident scalars; uses bases[offset .. offset+n) -- the shard primitive for
 * multi-GPU runs (each rank owns a slice of the points, then pm_g1_fold after all-gather).
 * Blocks until the 144-byte result is on the host. */
int pm_g1_msm_dev(pm_ctx* ctx, const pm_bases* bases, size_t offset, size_t n,
                  const void* d_scalars, uint32_t scalar_form, uint64_t out_xyz[18],
                  void* hip_stream);

/* `batch` MSMs over the SAME bases in one pass (a prover round commits to 4-6 polynomials of one
 * size): scalar vector j starts at d_scalars + 32 * j * scalar_stride, result j at out_xyz + 18 j.
 * The sort and the additions scale with the batch, the latency-bound tail (bucket reduction, host
 * fold) is paid once.  batch <= 64. */
int pm_g1_msm_batch_dev(pm_ctx* ctx, const pm_bases* bases, size_t offset, size_t n, const void* d_scalars,
                        size_t scalar_stride, uint32_t batch, uint32_t scalar_form, uint64_t* out_xyz,
                        void* hip_stream);

/* out[i] = scalars[i] * base for device-resident scalars; affine results (n x 96 bytes, (0, 0) =
 * identity) in device memory.  SRS generation: with scalars = tau^i
 * (pm_fr_powers_dev) this is the powers_of_g of dusk_plonk's PublicParameters::setup, which upstream
 * computes on the CPU with a windowed single-base multiplication.  Blocks until done. */
int pm_g1_fixed_base_mul_dev(pm_ctx* ctx, const uint64_t base_xy[12], const void* d_scalars, size_t n,
                             uint32_t scalar_form, void* d_out_xy, void* hip_stream);

/* Lagrange-form commit key: out[i] = [L_i(tau)]G = n^-1 sum_{j<n} w^-ij powers[j], n = 2^log_n <= pm_g1_bases_len(powers),
 * written to d_out_xy (n x 96 bytes, ABI affine) -- hand it to pm_g1_bases_from_dev.  Any points are accepted (it is
 * the inverse NTT of the first n bases); identities allowed.  PM_ERR_LENGTH when n exceeds the bases,
 * PM_ERR_DOMAIN_TOO_LARGE when log_n >= 32.  Allocates n x 320 + n x 32 bytes of scratch for the call; blocks until done. */
int pm_g1_bases_lagrange(pm_ctx* ctx, const pm_bases* powers, uint32_t log_n, void* d_out_xy, void* hip_stream);

/* ---- Per-point scalar multiplication -------------------------------------------------------
 * out[i] = scalars[i] * points[i]: `G1Affine * Scalar` of dusk_bls12_381 in bulk, one thread per point.  Points and
 * results are ABI affine (n x 96 bytes, Montgomery R = 2^384, (0, 0) = identity); scalars are n x 32 bytes in either
 * PM_SCALAR_* form, below r.  A zero scalar or an identity point gives (0, 0).  d_out_xy == d_points_xy is allowed.
 * flags = 0: a signed-window ladder over the whole scalar, valid for ANY point of the curve.
 * PM_G1_POINTS_IN_SUBGROUP: the caller asserts that every point is the identity or has order r (a key from
 * pm_g1_bases_from_compressed with PM_G1_CHECK_SUBGROUP, or one that passed pm_g1_check_dev / pm_g1_bases_check with it);
 * the scalar is split k = k1 + k2 z^2 and the ladder runs over the two 128-bit halves with the endomorphism
 * (x, y) -> (beta x, -y) = [z^2] P.  RESULTS UNDER THE FLAG ARE UNDEFINED FOR POINTS OUTSIDE THE SUBGROUP (the library
 * does not check; a curve point of another order gives a wrong point, silently).
 * n == 0 is PM_OK; null pointers, an unknown scalar form and unknown flag bits are PM_ERR_BAD_ARG.  Allocates n x 320
 * bytes of scratch plus a window table (1792 bytes per thread in flight, at most 256 MiB) for the call; blocks until
 * done. */
#define PM_G1_POINTS_IN_SUBGROUP 1u /* caller asserts: every point is the identity or has order r */
int pm_g1_scalar_mul_dev(pm_ctx* ctx, const void* d_points_xy, const void* d_scalars, size_t n, uint32_t scalar_form,
                         uint32_t flags, void* d_out_xy, void* hip_stream);
/* pm_g1_bases_lagrange with flags: 0 is exactly that call.  With PM_G1_POINTS_IN_SUBGROUP (same assertion, same caveat:
 * undefined for points outside the subgroup) the twiddle multiplications take the split ladder; the bytes written are
 * the same.  Unknown flag bits: PM_ERR_BAD_ARG. */
int pm_g1_bases_lagrange_ex(pm_ctx* ctx, const pm_bases* powers, uint32_t log_n, uint32_t flags, void* d_out_xy,
                            void* hip_stream);
/* The inverse of pm_g1_bases_from_dev: the resident bases as ABI affine points (pm_g1_bases_len x 96 bytes) written to
 * d_out_xy on the stream; the input of pm_g1_scalar_mul_dev for a key that never leaves the device.  Asynchronous. */
int pm_g1_bases_to_dev(pm_ctx* ctx, const pm_bases* bases, void* d_out_xy, void* hip_stream);

/* ---- Checked commit-key loading: compressed G1 and point checks ----------------------------
 * The 48-byte zcash encoding of G1Affine::{to_compressed, from_compressed} (dusk's CommitKey::to_var_bytes / from_slice
 * is n of them back to back): big-endian x; byte 0 bit 7 = compressed (must be set), bit 6 = infinity (then every other
 * bit must be zero), bit 5 = y is the root above (p - 1) / 2.  Decoding checks x < p and y^2 = x^3 + 4, and with
 * PM_G1_CHECK_SUBGROUP also [r]P = identity (the identity passes).  Points are ABI affine (x | y, Montgomery R = 2^384,
 * (0, 0) = identity).  A failed point gives PM_ERR_POINT; bad_index / bad_reason (either may be NULL) receive the LOWEST
 * failing index and, for that point, the lowest reason that applies -- the same on every run.  The output is always
 * written in full; a rejected point comes back as (0, 0).  n == 0 is PM_OK; null pointers and unknown flag bits are
 * PM_ERR_BAD_ARG. */
#define PM_G1_CHECK_SUBGROUP 1u
#define PM_G1_BAD_ENCODING 1u          /* malformed encoding, or a coordinate that is not below p */
#define PM_G1_BAD_NOT_ON_CURVE 2u
#define PM_G1_BAD_NOT_IN_SUBGROUP 3u
/* Pure host, no context: one point (a proof's commitments, a verifier key). */
int pm_g1_compress(const uint64_t xy[12], uint8_t out[48]);
int pm_g1_decompress(const uint8_t in[48], uint32_t flags, uint64_t xy[12], uint32_t* bad_reason);
/* Device buffers (n x 48 bytes / n x 96 bytes); the checking calls block until the verdict is on the host. */
int pm_g1_decompress_dev(pm_ctx* ctx, const void* d_bytes, size_t n, uint32_t flags, void* d_out_xy, uint64_t* bad_index,
                         uint32_t* bad_reason, void* hip_stream);
/* Points already in ABI affine form (a key loaded raw): both coordinates below p and on the curve, or the pair (0, 0);
 * with PM_G1_CHECK_SUBGROUP also in the subgroup.  Reads only. */
int pm_g1_check_dev(pm_ctx* ctx, const void* d_xy, size_t n, uint32_t flags, uint64_t* bad_index, uint32_t* bad_reason,
                    void* hip_stream);
int pm_g1_compress_dev(pm_ctx* ctx, const void* d_xy, size_t n, void* d_bytes_out, void* hip_stream);
/* The same check on resident bases (pm_g1_bases_upload reduces coordinates mod p, so reason 1 cannot occur here). */
int pm_g1_bases_check(pm_ctx* ctx, const pm_bases* bases, uint32_t flags, uint64_t* bad_index, uint32_t* bad_reason);
/* CommitKey::from_slice: n x 48 host bytes -> resident bases; decoded and checked on the device, the points never visit
 * the host.  No pm_bases on failure (*out = NULL). */
int pm_g1_bases_from_compressed(pm_ctx* ctx, const uint8_t* bytes, size_t n, uint32_t flags, pm_bases** out,
                                uint64_t* bad_index, uint32_t* bad_reason);
/* CommitKey::to_var_bytes: the resident bases as pm_g1_bases_len(bases) x 48 host bytes. */
int pm_g1_bases_to_compressed(pm_ctx* ctx, const pm_bases* bases, uint8_t* bytes_out);

/* out = sum of k projective points (the group-law "all-reduce" after an all-gather). Host. */
int pm_g1_fold(const uint64_t* xyz_parts, size_t k, uint64_t out_xyz[18]);

/* Projective (homogeneous X/Z, Y/Z) -> affine; *is_identity = 1 and xy = 0 for infinity. */
int pm_g1_to_affine(const uint64_t xyz[18], uint64_t xy[12], int* is_identity);
/* k points ([k][18] -> [k][12], is_identity[k] optional) with one field inversion. */
int pm_g1_to_affine_batch(const uint64_t* xyz, size_t k, uint64_t* xy, int* is_identity);

/* ---- device-resident polynomial helpers (the callers either side of the hot path) ------- */
/* dusk_plonk::fft::{Polynomial, Evaluations} and
 * util::batch_inversion as used by the prover rounds between the NTT and MSM calls.  All
 * vectors are canonical Fr in DEVICE memory; `hip_stream` as in pm_fr_ntt_dev. */

/* Device memory for callers without their own HIP allocator (the Rust prover, the tests). */
int pm_dev_alloc(pm_ctx* ctx, size_t bytes, void** out);
int pm_dev_free(pm_ctx* ctx, void* p);
int pm_dev_upload(pm_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int pm_dev_download(pm_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* out[i] = a[i] (op) b[i]:  op 0 = add, 1 = sub, 2 = mul  (Evaluations / Polynomial `+ - *`).
 * b_len == 1 broadcasts one scalar (Polynomial * scalar).  In place allowed. */
int pm_fr_vec_op_dev(pm_ctx* ctx, int op, const void* d_a, const void* d_b, size_t b_len, void* d_out,
                     size_t n, void* hip_stream);
/* Polynomial::evaluate: out = sum_i coeffs[i] * point^i.  Blocks until `out` is on the host. */
int pm_fr_poly_evaluate_dev(pm_ctx* ctx, const void* d_coeffs, size_t n, const uint64_t point[4],
                            uint64_t out[4], void* hip_stream);
/* The same for k <= PM_LINCOMB_MAX polynomials of n coefficients at ONE point (d_polys: host array of device
 * pointers, out: k x 4 limbs): one pass of kernels and a single host synchronisation -- the prover opens
 * 15 polynomials at z and 4 at z w. */
int pm_fr_poly_evaluate_many_dev(pm_ctx* ctx, uint32_t k, const void* const* d_polys, size_t n, const uint64_t point[4],
                                 uint64_t* out, void* hip_stream);
/* Polynomial::ruffini: quotient of coeffs(X) / (X - z), n-1 coefficients into d_out (the
 * remainder coeffs(z) is dropped, as upstream).  Not in place.  Asynchronous on the stream. */
int pm_fr_poly_ruffini_dev(pm_ctx* ctx, const void* d_coeffs, size_t n, const uint64_t z[4], void* d_out,
                           void* hip_stream);
/* out[0] = 1, out[i] = in[0] * ... * in[i-1]: the grand-product accumulator z(X) of the permutation
 * argument (dusk_plonk::permutation).  In place allowed. */
int pm_fr_prefix_product_dev(pm_ctx* ctx, const void* d_in, size_t n, void* d_out, void* hip_stream);
/* util::batch_inversion: every non-zero element is replaced by its inverse, zeros stay zero. */
int pm_fr_batch_inverse_dev(pm_ctx* ctx, void* d_inout, size_t n, void* hip_stream);

/* ---- PLONK prover rounds (BASELINE.json configs[3]) ----------- */
/* The pointwise work of dusk_plonk::proof_system::{permutation, quotient_poly, linearisation_poly}
 * (dusk-plonk 0.8.2, ref:Cargo.toml:19) for a 4-wire arithmetic circuit
 *   q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c + PI = 0
 * with copy constraints over the cosets {1, k1, k2, k3} H, fused into one kernel per round so that
 * every polynomial stays in HBM between the NTT and MSM calls.  Vectors are canonical Fr in device
 * memory; challenges and constants are host Fr (Montgomery limbs). */

/* out[i] = scale * base^i, i < n: domain.elements(), the 4n-coset points g w^i, powers of a challenge. */
int pm_fr_powers_dev(pm_ctx* ctx, const uint64_t base[4], const uint64_t scale[4], size_t n, void* d_out,
                     void* hip_stream);

/* out = sum_j coeffs[j] * vecs[j], k <= PM_LINCOMB_MAX vectors of n elements (d_vecs: host array of
 * device pointers): the linearisation polynomial and the aggregated opening polynomial. */
#define PM_LINCOMB_MAX 16
int pm_fr_lincomb_dev(pm_ctx* ctx, uint32_t k, const void* const* d_vecs, const uint64_t* coeffs, size_t n,
                      void* d_out, void* hip_stream);

/* Permutation argument, per row i < n of the domain H (x_i = roots[i] = w^i):
 *   num[i] = prod_j (wires[j][i] + beta k_j x_i + gamma),   k_0 = 1
 *   den[i] = prod_j (wires[j][i] + beta sigmas[j][i] + gamma)
 * z = prefix_product(num / den) (pm_fr_batch_inverse_dev, pm_fr_vec_op_dev, pm_fr_prefix_product_dev). */
typedef struct pm_plonk_perm_args {
  const void* wires[4];   /* a, b, c, d evaluations on H */
  const void* sigmas[4];  /* sigma_1..4 evaluations on H */
  const void* roots;      /* w^i */
  uint64_t beta[4], gamma[4];
  uint64_t k[3][4];       /* coset representatives k1, k2, k3 (dusk: 7, 13, 17) */
} pm_plonk_perm_args;
int pm_plonk_perm_terms_dev(pm_ctx* ctx, const pm_plonk_perm_args* args, size_t n, void* d_num, void* d_den,
                            void* hip_stream);

/* Quotient numerator divided by Z_H, pointwise on the 4n coset (x_i = g w_4n^i, i < 4n):
 *   t[i] = zh_inv[i mod 4] * ( q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c) + pi
 *          + q_range R + q_logic L + q_fixed_group_add F + q_variable_group_add V
 *          + alpha   ( z[i]   prod_j (w_j + beta k_j x_i + gamma)
 *                    - z[i+4] prod_j (w_j + beta sigma_j + gamma) )
 *          + alpha^2 ( z[i] - 1 ) l1[i] )
 * (index i+4 wraps: f(w X) on the 4n coset).  R, L, F, V are dusk-plonk 0.8's widget identities
 * (proof_system::widget::{range, logic, ecc::scalar_mul::fixed_base, ecc::curve_addition}) over the
 * row's wires and a_next, b_next, d_next, each times its separation challenge:
 *   R = s (delta(c - 4d) + k delta(b - 4c) + k^2 delta(a - 4b) + k^3 delta(d_next - 4a)),  k = s^2,
 *       delta(f) = f (f-1)(f-2)(f-3)
 *   L = s (delta(qa) + k delta(qb) + k^2 delta(qd) + k^3 (c - qa qb) + k^4 delta_xor_and(qa, qb, c, qd, q_c)),
 *       qa = a_next - 4a, qb = b_next - 4b, qd = d_next - 4d
 *   F = one round of JubJub fixed-base scalar multiplication (table point in q_l, q_r, q_c)
 *   V = JubJub addition (a, b) + (c, d) = (a_next, b_next), d_next = a d
 * coset_ifft of t gives the quotient polynomial.  A NULL q_arith means the constant 1, a NULL widget
 * selector means identically zero (that widget is not evaluated). */
typedef struct pm_plonk_quotient_args {
  const void* wires[4];
  const void* z;
  const void* q_m;
  const void* q_l;
  const void* q_r;
  const void* q_o;
  const void* q_4;
  const void* q_c;
  const void* pi;         /* public-input polynomial on the coset */
  const void* sigmas[4];
  const void* l1;         /* first Lagrange polynomial on the coset */
  const void* x;          /* the coset points g w_4n^i */
  uint64_t alpha[4], beta[4], gamma[4];
  uint64_t k[3][4];
  uint64_t zh_inv[4][4];  /* 1 / (x_i^n - 1), which only depends on i mod 4 */
  const void* q_arith;                /* NULL = 1 */
  const void* q_range;                /* NULL = 0, as the three below */
  const void* q_logic;
  const void* q_fixed_group_add;
  const void* q_variable_group_add;
  uint64_t range_sep[4], logic_sep[4], fixed_sep[4], var_sep[4];   /* the widgets' separation challenges */
} pm_plonk_quotient_args;
int pm_plonk_quotient_dev(pm_ctx* ctx, const pm_plonk_quotient_args* args, size_t n, void* d_out,
                          void* hip_stream);

/* ---- the whole prover behind one call ------------------------------------------------------------ */
/* Prover::{preprocess, prove_with_preprocessed} of dusk-plonk 0.8.2 (ref:Cargo.toml:19) sequenced inside the
 * library: 11 selector polynomials (the gate kinds the reference's gadgets emit: arithmetic, range, logic,
 * fixed-base scalar multiplication, variable-base curve addition -- ref:src/zk/gadgets.rs:34,37,40,88-91,211),
 * the 4-wire permutation, five rounds, 11 commitments, the 16 evaluations of dusk's Proof, a Merlin
 * transcript seeded with the verifier key.  Transcript (labels restated from the published 0.8 design,
 * unpinned): Transcript::new(label); q_m q_l q_r q_o q_c q_4 q_arith q_range q_logic q_variable_group_add
 * q_fixed_group_add left_sigma right_sigma out_sigma fourth_sigma; "dom-sep" = "circuit_size", "n";
 * w_l w_r w_o w_4; beta (re-absorbed), gamma; z; alpha and the four "... separation challenge"s; t_1..t_4;
 * z; the 17 "<name>_eval" scalars; "aggregate_witness" twice; w_z, w_z_w. */
#define PM_PLONK_SELECTORS 11   /* q_m q_l q_r q_o q_c q_4 q_arith q_range q_logic q_fixed_group_add q_variable_group_add */
#define PM_PLONK_VK_POINTS 15   /* the selector commitments in that order, then sigma_1..4 */
#define PM_PLONK_EVALS 17       /* a b c d a_next b_next d_next sigma_1 sigma_2 sigma_3 q_arith q_c q_l q_r z_next t r */
#define PM_PLONK_CHALLENGES 10  /* beta gamma alpha range_sep logic_sep fixed_sep var_sep z aw aw_shifted */
#define PM_PLONK_PROOF_BYTES 1040
/* prove flags.  DEFAULT (flags = 0): the public inputs (count, then position and value of every DECLARED input --
 * pass the positions of zero-valued inputs too) are absorbed into the transcript before round 1, so the statement is
 * bound to every challenge.  dusk-plonk 0.8.2 does not do that (its transcript never sees the public inputs):
 * PM_PLONK_UPSTREAM_TRANSCRIPT reproduces the restated upstream message sequence byte for byte and is what a drop-in
 * for dusk's Prover must pass ("Transcript modes").  The two modes agree up to and including the
 * four wire commitments and differ from `beta` on.  PM_PLONK_BIND_PUBLIC_INPUTS (r01/r02 spelling of the default) is
 * accepted and ignored; both flags together contradict each other: PM_ERR_BAD_ARG.
 * CHANGE r03: up to r02 flags = 0 meant the upstream sequence and binding was opt-in; a C caller that passed 0 and
 * needs the r02 bytes must now pass PM_PLONK_UPSTREAM_TRANSCRIPT. */
#define PM_PLONK_BIND_PUBLIC_INPUTS 1u
#define PM_PLONK_UPSTREAM_TRANSCRIPT 2u
typedef struct pm_prover_key pm_prover_key;
typedef struct pm_plonk_proof {
  uint64_t commitments[11][12];                  /* a b c d z t_1 t_2 t_3 t_4 w_z w_zw, affine, (0, 0) = identity */
  uint64_t evaluations[PM_PLONK_EVALS][4];       /* transcript order (above), Montgomery limbs; t is not part of dusk's Proof */
  uint64_t challenges[PM_PLONK_CHALLENGES][4];   /* recomputable from the transcript */
} pm_plonk_proof;
/* ProverKey: selectors[s] = n evaluations on H (host memory) in the order of PM_PLONK_SELECTORS, NULL =
 * identically zero; sigma_index[j n + i] = position (j' n + i') that follows wire j of gate i in its copy
 * cycle.  n a power of two >= 4.  Builds the coefficient forms, the 4n-coset forms the quotient needs
 * (trivial selectors -- q_arith = 1, a widget selector = 0 -- are recognised and skipped) and the per-proof
 * workspace (about 90 n x 32 bytes). */
int pm_plonk_preprocess(pm_ctx* ctx, const uint64_t* const selectors[PM_PLONK_SELECTORS], const int64_t* sigma_index,
                        size_t n, pm_prover_key** out);
void pm_plonk_key_free(pm_ctx* ctx, pm_prover_key* key);
/* Commits to the 15 polynomials of the key (the G1 part of dusk's VerifierKey) and seeds the key's base
 * transcript with them (Prover::preprocess).  Must run once before the first proof; commit_key: at least n
 * resident bases.  verifier_key_out: PM_PLONK_VK_POINTS affine points, may be NULL.  transcript_label NULL =
 * "plonk". */
int pm_plonk_key_commit(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key, const char* transcript_label,
                        uint64_t (*verifier_key_out)[12]);
int pm_plonk_verifier_key(const pm_prover_key* key, uint64_t (*out)[12]);
/* Round-1 wire commitments from the witness over a Lagrange-form key (NULL detaches).  lagrange must hold exactly n
 * points (PM_ERR_LENGTH otherwise) and is checked once against commit_key: sum_i L_i = powers[0] and
 * sum_i w^i L_i = powers[1] (two MSMs); PM_ERR_BAD_ARG if either fails.  pm_plonk_prove on this key then requires the
 * same commit_key (PM_ERR_BAD_ARG otherwise); pm_plonk_prove_sharded ignores the attachment.  The caller keeps
 * ownership: lagrange must outlive the attachment.  The proof bytes are those of a key without the attachment. */
int pm_plonk_key_set_lagrange(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key, const pm_bases* lagrange);
/* d_witness: device memory, [a | b | c | d] wire values, 4n Fr.  Public inputs: n_pi (position < n, value)
 * pairs in host memory -- the dense PI vector of dusk's construct_dense_pi_vec is built on the device.
 * commit_key: at least n resident bases (pm_g1_bases_upload / pm_g1_bases_from_dev, ideally with
 * pm_g1_bases_precompute).  One proof at a time per key (PM_ERR_BUSY otherwise). */
int pm_plonk_prove(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key, const void* d_witness,
                   const uint64_t* pi_positions, const uint64_t* pi_values, size_t n_pi, uint32_t flags,
                   pm_plonk_proof* out);
/* ---- Zero-knowledge proofs -----------------------------------------------------------------
 * pm_plonk_prove_zk makes a proof in the same format, transcript and challenge derivation as pm_plonk_prove (the
 * verifier does not change) whose wires, permutation polynomial and quotient pieces are blinded with the caller's
 * PM_PLONK_ZK_BLINDERS scalars b[0..16] (Montgomery limbs like the witness, each below r; Z_H = X^n - 1):
 *   a, b, d   w + (b_k + b_{k+1} X + b_{k+2} X^2) Z_H     a: k = 0, b: k = 3, d: k = 8
 *   c         c + (b_6 + b_7 X) Z_H
 *   z         z + (b_11 + b_12 X + b_13 X^2) Z_H
 *   t pieces  t_1 + b_14 X^n,  t_2 - b_14 + b_15 X^n,  t_3 - b_15 + b_16 X^n,  t_4 - b_16
 * The blinded quotient has degree up to 4n + 9, so t_4 holds n + 10 coefficients and the commit key needs at least
 * n + PM_PLONK_ZK_EXTRA_BASES resident bases (PM_ERR_LENGTH otherwise).  Blinders must be fresh uniform scalars for every
 * proof (fixed blinders are for tests only).
 * pm_plonk_key_enable_zk (committed key; idempotent) builds the key's second 4n coset 7 w_8n H_4n -- selectors, sigmas
 * and L_1 there -- and the padded per-proof workspace; added_bytes (may be NULL) receives the device bytes the zero-
 * knowledge state holds, the same figure on every call.  pm_plonk_prove_zk takes the flags of pm_plonk_prove and uses a
 * Lagrange key attached to the key (the proof is byte-identical without it).  With all blinders zero the proof is
 * byte-identical to pm_plonk_prove's.  Errors: key not enabled, NULL or non-canonical blinders, bad flags:
 * PM_ERR_BAD_ARG; a short commit key: PM_ERR_LENGTH; a key in use: PM_ERR_BUSY.  Single GPU only; pm_plonk_prove
 * on an enabled key is unchanged. */
#define PM_PLONK_ZK_BLINDERS 17
#define PM_PLONK_ZK_EXTRA_BASES 10
int pm_plonk_key_enable_zk(pm_ctx* ctx, pm_prover_key* key, size_t* added_bytes);
int pm_plonk_prove_zk(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key, const void* d_witness,
                      const uint64_t* pi_positions, const uint64_t* pi_values, size_t n_pi, uint32_t flags,
                      const uint64_t (*blinders)[4], pm_plonk_proof* out);
/* ---- Many proofs of one circuit in one call -----------------------------------------------------------------------
 * A batch workspace holds the per-proof polynomials of up to max_batch proofs on one committed key (about 42 n x 32 bytes
 * per proof, one device allocation; PM_ERR_OOM when it does not fit).  The key's own workspace and busy flag are not
 * used: only its read-only data is shared, so pm_plonk_prove on the key may run beside a batch (on another context).
 * pm_plonk_prove_batch proves `batch` witnesses together: d_witnesses is device memory, batch x [a | b | c | d] x n Fr,
 * proof-major; proof b's public inputs are the n_pi[b] pairs (pi_positions[b][i] < n, pi_values[b] + 4 i), and n_pi
 * (or pi_positions / pi_values) may be NULL for a batch without public inputs.  out[b] is byte-identical, challenges
 * included, to pm_plonk_prove of witness b with the same public inputs and flags, also with a Lagrange key attached to
 * the key.  Errors: batch 0 or above max_batch, a workspace of another key, an uncommitted key, contradicting flags:
 * PM_ERR_BAD_ARG; a position >= n: PM_ERR_LENGTH; a workspace in use: PM_ERR_BUSY.  Single GPU only. */
typedef struct pm_plonk_batch pm_plonk_batch;
#define PM_PLONK_MAX_BATCH 64
int pm_plonk_batch_create(pm_ctx* ctx, const pm_prover_key* key, uint32_t max_batch, pm_plonk_batch** out);
void pm_plonk_batch_free(pm_ctx* ctx, pm_plonk_batch* ws);
size_t pm_plonk_batch_bytes(const pm_plonk_batch* ws);   /* device bytes the workspace holds */
int pm_plonk_prove_batch(pm_ctx* ctx, pm_prover_key* key, pm_plonk_batch* ws, const pm_bases* commit_key, uint32_t batch,
                         const void* d_witnesses, const uint64_t* const* pi_positions, const uint64_t* const* pi_values,
                         const size_t* n_pi, uint32_t flags, pm_plonk_proof* out);
/* ---- Zero-knowledge proofs in a batch ------------------------------------------------------
 * pm_plonk_batch_enable_zk adds the padded-stride, per-proof regions of zero-knowledge batches for max_batch proofs to a
 * workspace, in one further device allocation (about 51 n x 32 bytes per proof).  The key must have had
 * pm_plonk_key_enable_zk: it owns the second-coset forms all proofs share.  Idempotent; added_bytes (may be NULL) receives
 * the bytes added, the same figure on every call, which pm_plonk_batch_zk_bytes reports too (0 before the call;
 * pm_plonk_batch_bytes keeps counting the plain regions only).  PM_ERR_OOM when it does not fit: the workspace stays
 * usable for plain batches.  An enabled workspace serves pm_plonk_prove_batch with unchanged proofs.
 * pm_plonk_prove_batch_zk takes the arguments of pm_plonk_prove_batch and batch x PM_PLONK_ZK_BLINDERS blinders
 * (blinders[b][i]: Montgomery limbs, below r).  out[b] is byte-identical, challenges included, to pm_plonk_prove_zk of
 * witness b with public inputs b and blinders[b], also with a Lagrange key attached to the key.  Every proof needs its own
 * fresh uniform blinders: one set shared by a batch, or reused across calls, gives the witnesses away.  Errors: those of
 * pm_plonk_prove_batch; NULL blinders, a blinder not below r, a workspace without pm_plonk_batch_enable_zk:
 * PM_ERR_BAD_ARG; a commit key with fewer than n + PM_PLONK_ZK_EXTRA_BASES bases: PM_ERR_LENGTH; a workspace in use:
 * PM_ERR_BUSY.  Single GPU only. */
int pm_plonk_batch_enable_zk(pm_ctx* ctx, pm_plonk_batch* ws, size_t* added_bytes);
size_t pm_plonk_batch_zk_bytes(const pm_plonk_batch* ws);
int pm_plonk_prove_batch_zk(pm_ctx* ctx, pm_prover_key* key, pm_plonk_batch* ws, const pm_bases* commit_key, uint32_t batch,
                            const void* d_witnesses, const uint64_t* const* pi_positions, const uint64_t* const* pi_values,
                            const size_t* n_pi, uint32_t flags, const uint64_t (*blinders)[PM_PLONK_ZK_BLINDERS][4],
                            pm_plonk_proof* out);
/* ---- Witness check -------------------------------------------------------------------------
 * The provers accept any witness: with one wrong wire value the quotient no longer divides by Z_H and the call still
 * returns PM_OK and a well-formed proof that no verifier accepts.  pm_plonk_check_witness evaluates every identity of
 * pm_plonk_quotient_args on the rows of H instead of the 4n coset, one kernel, and names the rows that fail and why
 * (dusk-plonk: Composer::check_circuit_satisfied).  Row i, with a_next, b_next, d_next from row (i + 1) mod n and the
 * selectors at row i, gets the mask
 *   PM_PLONK_FAIL_ARITH       q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c) + PI_i != 0
 *   PM_PLONK_FAIL_RANGE       q_range != 0 and one of the four delta(.) summands of R is != 0
 *   PM_PLONK_FAIL_LOGIC       q_logic != 0 and one of the five summands of L is != 0
 *   PM_PLONK_FAIL_FIXED_BASE  q_fixed_group_add != 0 and one of the four summands of F is != 0
 *   PM_PLONK_FAIL_VAR_BASE    q_variable_group_add != 0 and one of the three summands of V is != 0
 *   PM_PLONK_FAIL_COPY        for some wire j, w[j n + i] != w[sigma_index[j n + i]]
 * The summands are what the separation challenge's powers join in R, L, F, V above: each is tested on its own, so the
 * check takes no challenge and is exact ("the gate sum vanishes for every choice of the separation challenges").
 * pm_plonk_key_enable_check (opt-in, idempotent; needs neither a commit key nor pm_plonk_key_commit) builds what the
 * check reads: the non-trivial selectors on H (one batched forward transform of the key's coefficient forms), the 4n
 * permutation indices as 32-bit words, and scratch of its own (dense public inputs, row masks, counters; grown to the
 * largest batch seen) -- a check never touches the per-proof workspace and has its own busy flag.  The key keeps only
 * sigma's field values, so the caller passes sigma_index again; it is verified against the key (the sigma values are
 * recomputed from it and compared on the device): PM_ERR_BAD_ARG when it is another permutation.  added_bytes (may be
 * NULL) receives the device bytes the state holds after the call; pm_plonk_key_free frees it.
 * pm_plonk_check_witness takes the witness and public inputs of pm_plonk_prove (canonical Montgomery limbs) and returns
 * PM_OK whenever the check ran, satisfied or not: the report carries the result, every field of it deterministic.
 * row_mask_out (host, n bytes, may be NULL) receives the mask of every row.  pm_plonk_check_witness_batch takes the
 * witnesses and public inputs of pm_plonk_prove_batch (1 <= batch <= PM_PLONK_MAX_BATCH); reports[b] and row b of
 * row_masks_out (batch x n bytes, may be NULL) equal the single call on witness b.  Errors: key not enabled, NULL
 * arguments, a batch out of range: PM_ERR_BAD_ARG; a position >= n: PM_ERR_LENGTH; a check already running on the key:
 * PM_ERR_BUSY.  Single GPU only. */
#define PM_PLONK_FAIL_ARITH 1u
#define PM_PLONK_FAIL_RANGE 2u
#define PM_PLONK_FAIL_LOGIC 4u
#define PM_PLONK_FAIL_FIXED_BASE 8u
#define PM_PLONK_FAIL_VAR_BASE 16u
#define PM_PLONK_FAIL_COPY 32u
typedef struct pm_plonk_witness_report {
  uint64_t failed_rows;   /* rows with a non-zero mask */
  uint64_t first_row;     /* the lowest failing row; UINT64_MAX when no row fails */
  uint32_t first_mask;    /* that row's mask; 0 when no row fails */
  uint32_t reserved;      /* 0 */
  uint64_t count[6];      /* count[k]: rows with bit k set */
} pm_plonk_witness_report;
int pm_plonk_key_enable_check(pm_ctx* ctx, pm_prover_key* key, const int64_t* sigma_index, size_t* added_bytes);
int pm_plonk_check_witness(pm_ctx* ctx, pm_prover_key* key, const void* d_witness, const uint64_t* pi_positions,
                           const uint64_t* pi_values, size_t n_pi, pm_plonk_witness_report* out, uint8_t* row_mask_out);
int pm_plonk_check_witness_batch(pm_ctx* ctx, pm_prover_key* key, uint32_t batch, const void* d_witnesses,
                                 const uint64_t* const* pi_positions, const uint64_t* const* pi_values, const size_t* n_pi,
                                 pm_plonk_witness_report* reports, uint8_t* row_masks_out);
/* ---- Composer-form circuits: the permutation and the witness from wire variables ------------
 * A constraint system holds four lists of variable ids per gate (dusk-plonk's w_l, w_r, w_o, w_4) and one assignment per
 * variable, not a ready-made permutation and 4n dense wire values.  These calls take that form.
 * wire_vars[j n + i] = the variable at wire j of gate i (the layout of the witness), an id in [0, num_vars) or
 * PM_PLONK_NO_VAR.  The copy permutation is DEFINED as: the positions of a variable, ordered by rank r = 4 i + j (gate
 * first, then a, b, c, d -- the order in which dusk's Permutation pushes Left(i), Right(i), Output(i), Fourth(i)), each
 * map to the next one, the last to the first; a variable that occurs once maps to itself.  sigma_index is a pure function
 * of wire_vars (a stable radix sort on the device, no ordering from atomics): the verifier key depends on it byte for
 * byte.  A PM_PLONK_NO_VAR position belongs to no copy class: sigma fixes it and its wire value is 0 -- dusk's padding
 * row (upstream's pad extends the wire lists with the zero variable without entering them in the variable map; restated
 * from the public design and PARITY-UNPINNED, like the transcript labels).
 * pm_plonk_sigma_from_wires: host in, host out (sigma_index_out: 4n x int64, the meaning pm_plonk_preprocess gives it);
 * the _dev form takes and leaves device memory and has synchronised `stream` (NULL = the context's) when it returns.
 * Scratch (two pair buffers and counts, about 64 n bytes) is freed before return.  An id that is >= num_vars and not
 * PM_PLONK_NO_VAR: PM_ERR_BAD_ARG, pm_last_error names the lowest such position.  n <= 2^29, num_vars < 2^32.
 * pm_plonk_preprocess_wires is pm_plonk_preprocess with the permutation given as wire_vars (host): sigma_index is built on
 * the device and goes straight into the key; the key keeps the wire map on the device (16 n bytes) and is otherwise an
 * ordinary pm_prover_key -- commit, prove, zk, batch, Lagrange attachment and free work as on any key.
 * pm_plonk_key_enable_check on such a key accepts sigma_index = NULL and rebuilds the key's own permutation from its wire
 * map (on a key from pm_plonk_preprocess NULL stays PM_ERR_BAD_ARG).  pm_plonk_key_num_vars: 0 for a key built from
 * sigma_index.
 * pm_plonk_witness_from_vars_dev expands assignments into witnesses on the device: d_vars holds batch x var_stride Fr
 * (var_stride >= the key's num_vars), d_witness_out receives batch x 4n Fr, proof-major (what pm_plonk_prove_batch takes):
 * w[b][p] = vars[b][wire_vars[p]], zero at PM_PLONK_NO_VAR positions.  Values are copied verbatim, with no range check,
 * as the provers treat a dense witness.  Asynchronous on `stream` (NULL = the context's).
 * The distributed prover is not extended: a caller of pm_plonk_preprocess_dist gets sigma_index from
 * pm_plonk_sigma_from_wires and slices it itself.
 * Errors: n not a power of two >= 4 (or above 2^29): PM_ERR_LENGTH; NULL pointers, an id out of range, batch 0 or above
 * PM_PLONK_MAX_BATCH, var_stride < num_vars, a key that was not built from wires: PM_ERR_BAD_ARG. */
#define PM_PLONK_NO_VAR 0xffffffffu
int pm_plonk_sigma_from_wires(pm_ctx* ctx, const uint32_t* wire_vars, size_t num_vars, size_t n, int64_t* sigma_index_out);
int pm_plonk_sigma_from_wires_dev(pm_ctx* ctx, const void* d_wire_vars, size_t num_vars, size_t n, void* d_sigma_index_out,
                                  void* stream);
int pm_plonk_preprocess_wires(pm_ctx* ctx, const uint64_t* const selectors[PM_PLONK_SELECTORS], const uint32_t* wire_vars,
                              size_t num_vars, size_t n, pm_prover_key** out);
size_t pm_plonk_key_num_vars(const pm_prover_key* key);
int pm_plonk_witness_from_vars_dev(pm_ctx* ctx, const pm_prover_key* key, const void* d_vars, size_t var_stride,
                                   uint32_t batch, void* d_witness_out, void* stream);
/* ---- Gadget witnesses: fill widget rows from their inputs (DESIGN.md sections 7.2f to 7.2i) ---------------------------
 * In a composer-form circuit most variables are not inputs but the internal accumulators of the four widget gadgets.
 * These calls are the inverse of the witness check: given a gadget's inputs in the variable assignment, write the
 * variables that make its rows hold, on the device, in the layout pm_plonk_witness_from_vars_dev reads.
 * A gadget names its rows (first_row, count) and its input variables; what it writes are the variables the key's wire
 * map holds at the positions below (PM_PLONK_NO_VAR positions are skipped).  Rows are relative to first_row, wires
 * a b c d and the identities are those of pm_plonk_quotient_args.
 *   RANGE, m = count rows, value v = in_var[0]: acc_0 = 0, acc_(k+1) = 4 acc_k + quad_k over the 4m quads of v, most
 *     significant first.  Row i < m carries (a, b, c, d) = (acc_(4i+3), acc_(4i+2), acc_(4i+1), acc_(4i)), row m carries
 *     d = acc_(4m).  PM_PLONK_GADGET_TOO_WIDE when v >= 2^(8m).
 *   LOGIC, Q = count quads, inputs x = in_var[0], y = in_var[1], param 0 = AND, 1 = XOR: A, B, D are the accumulators of x,
 *     y and x op y quad by quad, most significant first.  Row k < Q carries (A_k, B_k, qx_k qy_k, D_k), row Q carries a =
 *     A_Q, b = B_Q, d = D_Q.  TOO_WIDE when an input >= 4^Q.
 *   FIXED_BASE, R = count rounds (<= PM_PLONK_GADGET_MAX_ROUNDS), scalar s = in_var[0].  The start point is READ from a, b
 *     of row 0 (the caller sets it; dusk uses the identity (0, 1)); the table point (x_b, y_b) of row k is the key's q_l,
 *     q_r there.  Digits are the width-2 non-adjacent form: with x = 3 s, e_j = bit_(j+1)(x) - bit_(j+1)(s), and row k
 *     uses bit_k = e_(R-1-k).  d_0 = 0, d_(k+1) = 2 d_k + bit_k (= (x >> (R-k+1)) - (s >> (R-k+1)), never negative);
 *     c_k = bit_k x_b y_b; (a_(k+1), b_(k+1)) = (a_k, b_k) + (bit_k x_b, bit_k^2 (y_b - 1) + 1) under the twisted Edwards
 *     law of JubJub, (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + k), (y1 y2 + x1 x2) / (1 - k)), k = d x1 x2 y1 y2.  The
 *     gadget writes d of rows 0..R, c of rows 0..R-1 and a, b of rows 1..R.  PM_PLONK_GADGET_SCALAR_TOO_LONG when some
 *     e_j with j >= R is non-zero (every s < r has at most 256 digits).  The rounds are summed in another order than they
 *     are defined in (a prefix scan): start and table points must lie on the curve, where the law is associative and
 *     complete; for other points the values written are deterministic and unspecified.
 *   CURVE_ADD (count ignored): reads (x1, y1, x2, y2) = a b c d of row 0 and writes a = x3, b = y3, d = x1 y2 in row 1.
 *     PM_PLONK_GADGET_DEGENERATE, with a = b = 0 written, when 1 +- d x1 x2 y1 y2 is zero (impossible on the curve).
 * Composed gadgets: what a circuit builds from plain arithmetic rows.  They claim no widget row and
 * have no trailing row; the identity of their rows is q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c + PI) = 0.
 * None of them reports: no input is refused.
 *   ARITH, count >= 1 rows, no in_var: for i = 0 .. count-1 in row order, read a, b, d of row i and then write
 *     c := q_m a b + q_l a + q_r b + q_4 d + q_c (the row's own coefficients; every row has q_o = -1 and a c variable), so a
 *     later row reads what an earlier row of the same gadget wrote.  PI is taken as ZERO: a row carrying a public input is not
 *     for this gadget.  One thread walks the rows of a gadget one after the other: it is meant for the short glue between
 *     gadgets (a difference, a product of two flags); independent runs should be SEPARATE gadgets of one level, which run in
 *     parallel.
 *   BITS, B = count bits (1 <= B <= PM_PLONK_COMPOSED_MAX_BITS), value v = in_var[0], 2B rows -- the loop of a bit
 *     decomposition.  Row 2k is the boolean gate of bit k: a = b = c = bit_k, q_m = 1, q_o = -1.  Row 2k+1 accumulates:
 *     a = bit_k, b = acc_(k-1), c = acc_k, q_l = 2^k, q_r = 1, q_o = -1.  Every coefficient not named is zero.  With V the
 *     canonical integer of v (below r): bit_k = (V >> k) & 1; acc_(-1) is READ from b of row 1 (a circuit usually puts its
 *     zero variable there); acc_k = acc_(-1) + (V mod 2^(k+1)).  The gadget writes a of row 2k and c of row 2k+1.  V >= 2^B
 *     is no error: it is what the circuit around the gadget detects (acc_(B-1) != v).
 *   MAYBE_EQUAL (count ignored, no in_var), 3 rows.  Row 0: c = u = a - b (q_l = 1, q_r = -1, q_o = -1).  Row 1: a = z,
 *     b = u, c = y = 1 - u z (q_m = -1, q_c = 1, q_o = -1).  Row 2: a = y, b = u, q_m = 1, q_o = 0 (y u = 0).  Every
 *     coefficient not named is zero.  The gadget reads a, b of row 0 and writes u to c of row 0, z = 1 / u (0 when u = 0)
 *     to a of row 1 and y to c of row 1: y is 1 when the two inputs are equal and 0 otherwise.
 * Permutation gadgets: the rows of a whole permutation, filled by one wave per gadget and proof.
 *   HADES (kind PM_PLONK_PERMUTATION_HADES), one Hades permutation of width PM_PLONK_HADES_WIDTH = 5, as a Poseidon sponge
 *     uses it.  count = R >= 1 rounds, param = F full rounds, F even and 0 <= F <= R; no in_var, nothing reported.  Round rho is
 *     FULL when rho < F / 2 or rho >= R - F / 2 and PARTIAL otherwise.  Every row is an arithmetic row with q_o = -1 and no
 *     public input, as for ARITH; every coefficient not named is zero.  The rows of a round, in order, on the state s[0..4]:
 *       round keys, 5 rows: row j has a = s[j], c = s'[j] = s[j] + q_c, q_l = 1, q_c = any value (the round constant); b
 *         and d are not read (q_r = q_4 = 0);
 *       s-box, 3 rows per word, for j = 0..4 in order in a full round and for j = 4 only in a partial one: with x = s'[j],
 *         (a = b = x, c = x2), (a = b = x2, c = x4), (a = x4, b = x, c = x5), each with q_m = 1; x5 replaces the word;
 *       matrix, 2 rows for each i = 0..4, v the state after the s-box: (a = v0, b = v1, d = v2, c = z_i) with q_l, q_r, q_4 =
 *         any values, then (a = v3, b = v4, d = z_i, c = o_i) with q_l, q_r = any values and q_4 = 1: the five coefficients are
 *         row i of the matrix, o[0..4] is the state of the next round.
 *     A full round has 30 rows and a partial one 18: the gadget claims 30 F + 18 (R - F) rows (dusk-hades: R = 67, F = 8,
 *     1302 rows).  It reads a of its first five rows (PM_PLONK_NO_VAR reads as zero; the five may alias) and writes c of
 *     every row, byte for byte what an ARITH run over the same rows writes.
 * Variable-base scalar multiplication, kind PM_PLONK_GADGET_VAR_BASE = 10 (8 and 9 are no kinds):
 *   dusk-plonk's variable_base_scalar_mul, one wave per gadget and proof.  count = R rounds, 1 <= R <=
 *     PM_PLONK_GADGET_MAX_ROUNDS (dusk: 252), param = 0, no in_var; 6 R rows, no trailing row.  Round k is rows 6k .. 6k+5:
 *       6k    doubling          (a, b, c, d) = (acc.x, acc.y, acc.x, acc.y)      q_variable_group_add != 0
 *       6k+1  its second row    (dbl.x, dbl.y, -, acc.x acc.y)                   selectors not looked at
 *       6k+2  select x          (bit_k, P.x, sx, -)   arithmetic, q_m = 1, q_o = -1: sx = bit_k P.x
 *       6k+3  select y          (bit_k, P.y, sy, -)   arithmetic, q_m = 1, q_l = -1, q_c = 1, q_o = -1: sy = bit_k P.y - bit_k + 1
 *       6k+4  addition          (dbl.x, dbl.y, sx, sy)                           q_variable_group_add != 0
 *       6k+5  its second row    (new.x, new.y, -, dbl.x sy)                      selectors not looked at
 *     with dbl = acc + acc and new = dbl + (sx, sy) under the affine law above, acc of round k + 1 = new of round k; every
 *     coefficient of a select row that is not named is zero.  bit_0 is the MOST significant bit: from the identity the last
 *     (a, b) is (sum_k bit_k 2^(R-1-k)) P, from a start point S it is 2^R S plus that.  The gadget READS the start point from
 *     a, b of row 0 (the caller sets it; dusk uses the identity (0, 1)), bit_k from a of row 6k+2 and P from b of rows 2 and
 *     3 (PM_PLONK_NO_VAR reads as zero).  It WRITES a, b, d of rows 6k+1 and 6k+5 and c of rows 6k+2 and 6k+3; c of rows
 *     6k+1 and 6k+5 (dusk's zero variable) is not touched.  The select rows are exactly bit P.x and bit P.y - bit + 1
 *     whatever value the bit variable has.  While every bit is 0 or 1 and no denominator 1 +- d x1 x2 y1 y2 vanishes, every
 *     byte equals what CURVE_ADD at rows 6k and 6k+4 and an ARITH run of 2 rows at 6k+2 write on 2R levels -- for ANY field
 *     elements as start point and P, on the curve or not (the chain runs in the order of the definition, in extended
 *     coordinates under the unified law, and is normalised with one inversion per lane).  PM_PLONK_GADGET_TOO_WIDE when a
 *     bit variable is neither 0 nor 1 (it counts as 0 in the chain); PM_PLONK_GADGET_DEGENERATE when a denominator vanishes
 *     (impossible on the curve); one report a gadget, TOO_WIDE first.  In both cases the select rows are still exact and
 *     the points and products written are deterministic and unspecified.
 * Gadgets of one level are independent and run together; levels run in rising order, so a gadget may read what a lower
 * level wrote.  Two gadgets of ONE level may name the same variable as an output only where the definitions give both the
 * same value (the zero variable in d of a range's and a fixed-base's row 0, say); any other overlap is a race.  A gadget's
 * inputs must not be among the outputs of its own level.  A failing gadget still writes: the values of its input cut to
 * the width it has.  Every byte written and every report field is a pure function of the inputs; values are canonical
 * Montgomery limbs.
 * pm_plonk_key_set_gadgets (a key from pm_plonk_preprocess_wires; replaces an earlier table, count = 0 clears it) checks
 * the table and keeps it on the device: one batched forward transform of the key's q_l, q_r, q_range, q_logic,
 * q_fixed_group_add and q_variable_group_add into transient scratch (6 n x 32 bytes), a kernel that tests the selector of
 * every claimed row (RANGE, LOGIC, FIXED_BASE: rows 0..count-1; CURVE_ADD: row 0) and gathers the table points of all
 * fixed-base rounds (64 bytes each).  A table that holds a composed kind transforms all eleven selectors instead (11 n x
 * 32 bytes of transient scratch) and tests on every row such a gadget claims: q_arith is non-zero and the four widget
 * selectors are zero; ARITH: q_o = -1 and c is a variable; BITS and MAYBE_EQUAL: every coefficient has exactly the value
 * given above and the wire map has the ids the layout implies (BITS: a = b = c on row 2k, a of row 2k+1 = a of row 2k, b of
 * row 2k+1 = c of row 2k-1 for k >= 1; MAYBE_EQUAL: b of rows 1 and 2 = c of row 0, a of row 2 = c of row 1), the written
 * positions being variables -- so a BITS or MAYBE_EQUAL gadget that is accepted is satisfied by what the fill writes,
 * provided the variables it reads (BITS: the value and b of row 1; MAYBE_EQUAL: a, b of row 0) are not among those it writes
 * and its written variables are distinct from one another: that is not tested and stays the caller's to keep.  The
 * same kernel gathers q_m q_l q_r q_4 q_c of all ARITH rows (160 bytes each, counted in added_bytes); BITS and MAYBE_EQUAL
 * keep nothing.  BITS: 1 <= count <= PM_PLONK_COMPOSED_MAX_BITS and in_var[0] < num_vars; rows are count (ARITH), 2 count
 * (BITS) and 3 (MAYBE_EQUAL).  HADES is checked like a composed kind (all eleven selectors): on every claimed row q_arith is
 * non-zero, the widget selectors are zero, q_o = -1, every coefficient the layout fixes has exactly that value, the wire map
 * has the ids the layout implies (a of a key row of round rho >= 1 = c of the row of o_j in round rho - 1; the s-box and
 * matrix rows read the c's named above) and c is a variable -- so an accepted gadget is satisfied by what the fill writes,
 * provided its written variables are distinct from one another and from the five inputs, which stays the caller's to keep.
 * The free coefficients are gathered per round (5 round keys and 25 matrix entries, 960 bytes) and so are the c ids of the
 * round's rows (30 ids, 120 bytes), so that the fill never walks the wire map: 1080 bytes a round, counted in added_bytes
 * (R = 67: 64,320 + 8,040 = 72,360 bytes); a table without a HADES gadget holds what it held.  HADES: count >= 1, param even
 * and <= count, at most 2^32 HADES rows in a table.  VAR_BASE also takes the all-eleven-selectors path and is tested round by
 * round: q_variable_group_add is non-zero on rows 6k and 6k+4; rows 6k+2 and 6k+3 have q_arith non-zero, no widget selector and
 * exactly the six coefficients above; the wire map has c = a and d = b on row 6k, a, b of row 6k+4 = a, b of row 6k+1, c, d of
 * row 6k+4 = c of rows 6k+2 and 6k+3, a of row 6k+3 = a of row 6k+2, b of rows 6k+2 and 6k+3 = b of rows 2 and 3, a, b of row
 * 6(k+1) = a, b of row 6k+5; and every written position is a variable -- so an accepted gadget is satisfied by what the fill
 * writes, provided its written variables are distinct from one another and from those it reads (start point, bits, P), which is
 * not tested and stays the caller's to keep.  It keeps nothing beyond its record: the fill reads the ids of its rows from the
 * key's wire map (a lane those of its own <= 4 rounds), so added_bytes grows by the 32 bytes of the record alone.  VAR_BASE:
 * 1 <= count <= PM_PLONK_GADGET_MAX_ROUNDS, param = 0; kinds 8 and 9 are refused as unknown.  PM_ERR_BAD_ARG, with pm_last_error naming the lowest offending gadget, for: levels
 * not in rising order, an unknown kind or param, rows (the trailing row included) outside [0, n), a claimed row whose
 * selector is zero, a used in_var >= num_vars, count = 0 or a fixed-base or variable-base count above PM_PLONK_GADGET_MAX_ROUNDS, a key
 * that was not built from wires.  After a refusal the key keeps the table it had.  added_bytes (may be NULL): the device
 * bytes the table holds.  pm_plonk_key_free frees it.
 * pm_plonk_fill_gadgets_dev fills batch x var_stride assignments in place (var_stride >= num_vars, 1 <= batch <=
 * PM_PLONK_MAX_BATCH), one launch per level and kind on `stream` (NULL = the context's).  reports (host, batch entries)
 * may be NULL: the call is then asynchronous; otherwise it waits for the stream.  One fill at a time per key.  Errors:
 * NULL arguments, no table, batch out of range, var_stride < num_vars: PM_ERR_BAD_ARG. */
#define PM_PLONK_GADGET_RANGE 0u
#define PM_PLONK_GADGET_LOGIC 1u
#define PM_PLONK_GADGET_FIXED_BASE 2u
#define PM_PLONK_GADGET_CURVE_ADD 3u
#define PM_PLONK_GADGET_MAX_ROUNDS 256u
#define PM_PLONK_GADGET_TOO_WIDE 1u
#define PM_PLONK_GADGET_SCALAR_TOO_LONG 2u
#define PM_PLONK_GADGET_DEGENERATE 3u
#define PM_PLONK_COMPOSED_ARITH 4u         /* kinds 4..6 of pm_plonk_gadget.kind */
#define PM_PLONK_COMPOSED_BITS 5u
#define PM_PLONK_COMPOSED_MAYBE_EQUAL 6u
#define PM_PLONK_COMPOSED_MAX_BITS 256u
#define PM_PLONK_PERMUTATION_HADES 7u      /* kind 7: count = rounds R, param = full rounds F */
#define PM_PLONK_HADES_WIDTH 5u
#define PM_PLONK_GADGET_VAR_BASE (10u)     /* kind 10: count = rounds R <= PM_PLONK_GADGET_MAX_ROUNDS; 8 and 9 are no kinds */
typedef struct pm_plonk_gadget {
  uint32_t kind, level;     /* gadgets of a level are independent; levels run in rising order */
  uint64_t first_row;
  uint32_t count;           /* RANGE: rows m (8m bits); LOGIC: quads Q; FIXED_BASE: rounds R; CURVE_ADD: ignored; HADES, VAR_BASE: rounds R */
  uint32_t param;           /* LOGIC: 0 = AND, 1 = XOR; HADES: full rounds F; otherwise 0 */
  uint32_t in_var[2];       /* RANGE: value; LOGIC: a, b; FIXED_BASE: scalar; unused = PM_PLONK_NO_VAR */
} pm_plonk_gadget;
typedef struct pm_plonk_gadget_report {
  uint64_t failed;        /* gadgets whose input did not fit */
  uint64_t first_gadget;  /* lowest failing index, UINT64_MAX if none */
  uint32_t first_reason;  /* PM_PLONK_GADGET_TOO_WIDE | _SCALAR_TOO_LONG | _DEGENERATE; 0 if none */
  uint32_t reserved;      /* 0 */
} pm_plonk_gadget_report;
int pm_plonk_key_set_gadgets(pm_ctx* ctx, pm_prover_key* key, const pm_plonk_gadget* gadgets, size_t count, size_t* added_bytes);
int pm_plonk_fill_gadgets_dev(pm_ctx* ctx, const pm_prover_key* key, void* d_vars, size_t var_stride, uint32_t batch,
                              pm_plonk_gadget_report* reports, void* stream);
/* Pure host, no context: the rows a gadget claims, its trailing row included (RANGE, LOGIC, FIXED_BASE: count + 1; CURVE_ADD:
 * 2; ARITH: count; BITS: 2 count; MAYBE_EQUAL: 3; HADES: 30 F + 18 (R - F); VAR_BASE: 6 R).  0 for NULL, an unknown kind and a count or param
 * that pm_plonk_key_set_gadgets refuses on its own: count 0 where a count is needed, a count above its kind's cap, HADES with
 * F odd or F > R. */
uint64_t pm_plonk_gadget_rows(const pm_plonk_gadget* g);
/* ---- Native Poseidon: the Hades permutation outside a circuit, a sponge, a Merkle tree -------------
 * The permutation is the one PM_PLONK_PERMUTATION_HADES lays out in rows, width 5: R >= 1 rounds, F of them full (F even,
 * F <= R; round rho is full when rho < F / 2 or rho >= R - F / 2); a round adds its five round keys, raises every word (full)
 * or the last word (partial) to the fifth power and multiplies by its matrix: new[i] = sum_j mds[i][j] s[j].
 * pm_hades_params: the constants of one permutation, an opaque handle that owns a small device table (36 bytes a constant).
 *   _create: ark = [R][5] round keys, mds = [n_mds][5][5] matrices with n_mds = 1 (one matrix for every round: dusk-hades) or
 *     n_mds = R (round rho has its own: what the gadget kind allows), canonical Montgomery limbs.  PM_ERR_BAD_ARG, with
 *     pm_last_error saying which, for R = 0, F odd, F > R, any other n_mds, a constant that is not below the modulus, NULL.
 *   _from_key: the constants of gadget `gadget_index` (the caller's index) of the key's current gadget table, which must be
 *     of kind PM_PLONK_PERMUTATION_HADES: a copy of the 30 coefficients a round that pm_plonk_key_set_gadgets gathered, so the
 *     native permutation computes what the rows of that gadget constrain; n_mds = R.  Waits for the context's stream.
 *     PM_ERR_BAD_ARG for another kind, a key without a table, an index out of range.  The handle does not refer to the key:
 *     it stays valid after the table is replaced or the key is freed.
 *   _info: any of the three outputs may be NULL.  _free waits for the device before it releases the table.
 * The device calls are asynchronous on `hip_stream` (NULL = the context's stream), take addresses on the context's GPU
 * (16-byte aligned) and canonical Montgomery elements, use no context scratch, and launch nothing for n = 0 (PM_OK).  `flags`
 * picks the kernel: PM_HADES_FORM_THREAD runs one permutation per lane (throughput), PM_HADES_FORM_WAVE lets 25 lanes
 * cooperate on one, two permutations a wave (latency), PM_HADES_FORM_AUTO takes WAVE for small n and THREAD from the measured
 * crossover on; any other value is PM_ERR_BAD_ARG.  The forms write identical bytes.
 *   pm_hades_permute_dev: n states of 5 elements (160 bytes each, contiguous), permuted in place.
 *   pm_poseidon_hash_dev: n messages of msg_len >= 1 elements, message i at element i * msg_stride (msg_stride >= msg_len),
 *     one element of output a message; d_out must not overlap d_msgs.  This is the project's MODELLED sponge of rate 4, the
 *     one tests/hades_model.py lays out as a circuit -- the state starts as (capacity, 0, 0, 0, 0); every chunk of up to four
 *     inputs is added to words 1..4, a chunk shorter than four also adds 1 to the word after its last input, one permutation
 *     follows each chunk; the hash is word 1 of the final state.  capacity = 0 reproduces the modelled circuit.  It is NOT
 *     claimed to be dusk-poseidon's sponge: its padding and constants are as unpinned here as the transcript labels are.
 *     Absorption and permutation run in one kernel; the state stays in registers across chunks.
 *   pm_poseidon_merkle_dev: a tree of arity 4 over 4^height leaves, 1 <= height <= PM_POSEIDON_MERKLE_MAX_HEIGHT.  A node is
 *     word 1 of the permutation of (capacity, c0, c1, c2, c3), its four children: the hash above of a message of four.
 *     d_tree receives levels 1..height one after the other -- level l has 4^(height - l) nodes, the root is last --
 *     (4^height - 1) / 3 elements that must not overlap the leaves.  One launch a level; AUTO chooses the form per level.
 *   pm_poseidon_merkle_paths_dev: for each of k leaf indices (uint64, device memory) the four children of every ancestor:
 *     out[j][l][c], l < height, c < 4, is node ((i >> 2l) & ~3) + c of level l (level 0 = the leaves), i = indices[j] -- the
 *     path node itself is child (i >> 2l) & 3.  k x height x 4 elements.  An index >= 4^height is refused with
 *     PM_ERR_BAD_ARG, pm_last_error naming the lowest offending position; finding that out takes one 8-byte readback, so this
 *     call WAITS for the stream.  Nothing is read for a refused index; the entries of the others are written.
 *   pm_poseidon_merkle_update_dev: leaves[indices[j]] = values[j] for k leaves, then every ancestor of
 *     a changed leaf is hashed again, each once, and nothing else is written: afterwards leaves and tree hold the bytes
 *     pm_poseidon_merkle_dev writes over the updated leaves, in both forms.  d_indices: k uint64 in device memory, STRICTLY
 *     ASCENDING; d_values: k elements; d_work: caller-owned, 16-byte aligned, at least _update_work_bytes(k) bytes (a pure host
 *     function; 0 for k = 0).  PM_ERR_BAD_ARG, pm_last_error naming the lowest offending position, for an index >= 4^height
 *     or not above its predecessor -- the test runs on the device before anything is written, and A REFUSED CALL CHANGES NO
 *     BYTE of leaves or tree.  Also refused: what pm_poseidon_merkle_dev refuses, k > 4^height, and d_values, d_indices or
 *     d_work overlapping leaves or tree.  One launch chain without a readback between levels (AUTO chooses the form per level
 *     by the bound min(k, 4^(height - l))); the call WAITS for the stream once, at the end, and reads verdict and count in one
 *     copy.  *hashed (may be NULL) receives the permutations run: sum over l = 1..height of |{ indices[j] >> 2l }|.
 *   pm_poseidon_merkle_verify_dev: folds k paths as _paths_dev writes them ([k][height][4] elements) to d_root (one element;
 *     the tree's last element serves) and writes k uint32 to d_status: PM_MERKLE_PATH_OK; PM_MERKLE_PATH_INDEX for an index
 *     >= 4^height (nothing of that path is read); PM_MERKLE_PATH_LINK + l for the lowest l < height at which the hash of
 *     path[l] is not its successor -- child (index >> 2(l + 1)) & 3 of path[l + 1], the root for l = height - 1.  A bad path
 *     is a result, not an error.  Asynchronous: no readback, no scratch; d_status must not overlap an input.
 * The two host forms need no context and no GPU (csrc/host_field.h): the same permutation and sponge for a one-off hash.
 * They return PM_ERR_BAD_ARG for what _create refuses, a non-canonical input, NULL and msg_len = 0. */
#define PM_HADES_FORM_AUTO 0u
#define PM_HADES_FORM_THREAD 1u
#define PM_HADES_FORM_WAVE 2u
#define PM_POSEIDON_MERKLE_MAX_HEIGHT 15u
typedef struct pm_hades_params pm_hades_params;
int pm_hades_params_create(pm_ctx* ctx, uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds,
                           uint32_t n_mds, pm_hades_params** out);
int pm_hades_params_from_key(pm_ctx* ctx, const pm_prover_key* key, size_t gadget_index, pm_hades_params** out);
int pm_hades_params_info(const pm_hades_params* params, uint32_t* rounds, uint32_t* full_rounds, uint32_t* n_mds);
void pm_hades_params_free(pm_ctx* ctx, pm_hades_params* params);
int pm_hades_permute_dev(pm_ctx* ctx, const pm_hades_params* params, void* d_states, size_t n, uint32_t flags, void* hip_stream);
int pm_poseidon_hash_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], const void* d_msgs,
                         size_t msg_len, size_t msg_stride, size_t n, void* d_out, uint32_t flags, void* hip_stream);
int pm_poseidon_merkle_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], const void* d_leaves,
                           uint32_t height, void* d_tree, uint32_t flags, void* hip_stream);
int pm_poseidon_merkle_paths_dev(pm_ctx* ctx, const void* d_leaves, const void* d_tree, uint32_t height, const void* d_indices,
                                 size_t k, void* d_out, void* hip_stream);
#define PM_MERKLE_PATH_OK 0u
#define PM_MERKLE_PATH_INDEX 1u
#define PM_MERKLE_PATH_LINK 2u
size_t pm_poseidon_merkle_update_work_bytes(size_t k);
int pm_poseidon_merkle_update_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], void* d_leaves,
                                  void* d_tree, uint32_t height, const void* d_indices, const void* d_values, size_t k,
                                  void* d_work, uint32_t flags, uint64_t* hashed, void* hip_stream);
int pm_poseidon_merkle_verify_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], const void* d_paths,
                                  const void* d_indices, size_t k, uint32_t height, const void* d_root, void* d_status,
                                  uint32_t flags, void* hip_stream);
int pm_hades_permute_host(uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds,
                          uint64_t state[20]);
int pm_poseidon_hash_host(uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds,
                          const uint64_t capacity[4], const uint64_t* msg, size_t msg_len, uint64_t out[4]);
/* ---- The append-only Poseidon tree: a tree of ledger height that stores only what is filled ---------
 * Arity 4, a fixed height H, 1 <= H <= PM_POSEIDON_LEDGER_MAX_HEIGHT (4^31 = 2^62 positions), the hash of pm_poseidon_merkle_dev.
 * Leaves are filled from position 0 upward; `count` is their number.  Level 0 is the leaves, level l stores the nodes
 * [0, ceil(count / 4^l)): those with a filled descendant.  Everything to the right is an empty subtree whose hash is a constant
 * of its level: Z_0 = empty_leaf, Z_(l+1) = hash(Z_l, Z_l, Z_l, Z_l); a child at or beyond the stored prefix of its level reads
 * as that level's Z, and the root of an empty tree is Z_H.  A tree whose 4^H positions are all filled holds, level by level, the
 * bytes pm_poseidon_merkle_dev writes with the same constants and capacity.
 * The handle, an opaque struct of the name pm_poseidon_ledger, owns one device slab with room for `reserve` leaves and their
 * ancestors (level l: ceil(reserve / 4^l) elements, the levels one after the other), a device table of Z_0 .. Z_H, a
 * one-element device root that is current after every call, its own copy of the Hades constants and of the capacity word -- it
 * does not refer to `params` after _create -- and the host's count and reserve.  One handle must not be used by two calls at a
 * time, and calls on it that change it must be ordered on one stream.
 *   _create: the Z_l are computed on the host (pm_hades_permute_host's rounds).  PM_ERR_BAD_ARG for height 0 or above 31, a
 *     capacity or empty leaf that is not canonical, NULL, reserve_leaves > 4^height.  reserve_leaves = 0 allocates no slab.
 *   _free waits for the device.  _info: any output may be NULL; device_bytes counts the slab, the Z table, the root and the
 *     constants.  _bytes is pure host: the slab of a reserve, 32 * sum over l = 0..H of ceil(reserve / 4^l); 0 for arguments
 *     _create refuses.  _empty_roots writes Z_0 .. Z_H, height + 1 elements, to host memory.
 *   _append_dev: d_values[0 .. k) become the leaves count .. count + k - 1 (a device copy), then level l = 1..H hashes exactly
 *     the nodes (count >> 2l) .. ((count + k - 1) >> 2l), one launch a level with the form AUTO picks for that level's exact
 *     number of nodes, and a copy of the new root to the handle's root element.
 *     *hashed (may be NULL) = the sum over l of the range sizes, known to the host: the call is asynchronous with no readback.
 *     If count + k > reserve the slab grows first to max(2 reserve, count + k), at most 4^H: the stored prefixes are copied
 *     device to device and the call WAITS for the stream.  k = 0: PM_OK, nothing launched.  PM_ERR_LENGTH for count + k > 4^H
 *     or k > 2^31 - 1; PM_ERR_BAD_ARG for flags above PM_HADES_FORM_WAVE, a NULL or misaligned d_values and one that overlaps
 *     the handle's device memory (the slab, the Z table, the root).  A refused call changes nothing.
 *   _truncate_dev, the rollback: new_count > count is PM_ERR_BAD_ARG; new_count = count is PM_OK with *hashed = 0; new_count =
 *     0 sets the root to Z_H, *hashed = 0; otherwise the H ancestors of leaf new_count - 1 are hashed again, *hashed = H.
 *     Asynchronous.  Stored bytes beyond the new prefixes are not cleared and are never read as data: an append after a
 *     truncate gives the bytes of a fresh ledger over the same leaves.
 *   _root_dev copies the root to d_root (one element) on the stream; _root copies it to the host and WAITS for the stream.
 *     An output of _root_dev or _paths_dev that overlaps the handle's device memory -- a _level pointer, say -- is
 *     PM_ERR_BAD_ARG: no call writes tree state through a caller's buffer.
 *   _level: the stored prefix of level l <= H: its address (valid until the slab next grows; NULL when nothing is stored) and
 *     its number of nodes.  Bytes beyond `nodes` are unspecified.
 *   _paths_dev: as pm_poseidon_merkle_paths_dev, [k][H][4] elements; a sibling beyond a stored prefix is its level's Z.  An
 *     index >= count is PM_ERR_BAD_ARG naming the lowest offending position; nothing is read for it, the other paths are
 *     written; the call WAITS for the stream.
 *   _verify_dev: pm_poseidon_merkle_verify_dev -- its kernels, its status words, its refusals -- for 1 <= height <= 31.  It
 *     needs no handle: the caller holds the constants, the capacity and a root. */
#define PM_POSEIDON_LEDGER_MAX_HEIGHT 31u
typedef struct pm_poseidon_ledger pm_poseidon_ledger;
int pm_poseidon_ledger_create(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], uint32_t height,
                              const uint64_t empty_leaf[4], uint64_t reserve_leaves, pm_poseidon_ledger** out);
void pm_poseidon_ledger_free(pm_ctx* ctx, pm_poseidon_ledger* ledger);
int pm_poseidon_ledger_info(const pm_poseidon_ledger* ledger, uint32_t* height, uint64_t* count, uint64_t* reserve_leaves,
                            size_t* device_bytes);
size_t pm_poseidon_ledger_bytes(uint32_t height, uint64_t reserve_leaves);
int pm_poseidon_ledger_empty_roots(const pm_poseidon_ledger* ledger, uint64_t* out);
int pm_poseidon_ledger_append_dev(pm_ctx* ctx, pm_poseidon_ledger* ledger, const void* d_values, size_t k, uint32_t flags,
                                  uint64_t* hashed, void* hip_stream);
int pm_poseidon_ledger_truncate_dev(pm_ctx* ctx, pm_poseidon_ledger* ledger, uint64_t new_count, uint32_t flags, uint64_t* hashed,
                                    void* hip_stream);
int pm_poseidon_ledger_root_dev(pm_ctx* ctx, const pm_poseidon_ledger* ledger, void* d_root, void* hip_stream);
int pm_poseidon_ledger_root(pm_ctx* ctx, const pm_poseidon_ledger* ledger, uint64_t out[4], void* hip_stream);
int pm_poseidon_ledger_level(const pm_poseidon_ledger* ledger, uint32_t level, void** d_ptr, uint64_t* nodes);
int pm_poseidon_ledger_paths_dev(pm_ctx* ctx, const pm_poseidon_ledger* ledger, const void* d_indices, size_t k, void* d_out,
                                 void* hip_stream);
int pm_poseidon_ledger_verify_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], const void* d_paths,
                                  const void* d_indices, size_t k, uint32_t height, const void* d_root, void* d_status,
                                  uint32_t flags, void* hip_stream);
/* ---- Native JubJub: scalar multiplications on the embedded curve outside a circuit ------------------
 * The curve is the one the FIXED_BASE, CURVE_ADD and VAR_BASE gadgets constrain: -x^2 + y^2 = 1 + d x^2 y^2 over Fr with
 * d = -(10240 / 10241), under the law (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + k), (y1 y2 + x1 x2) / (1 - k)),
 * k = d x1 x2 y1 y2.  A point is affine (x, y): two canonical Montgomery elements, 64 bytes; the identity is (0, 1).  The
 * multiplier of a point is the INTEGER 0 <= s < r its scalar stands for (scalar_form: PM_SCALAR_MONTGOMERY or
 * PM_SCALAR_CANONICAL, anything else is PM_ERR_BAD_ARG), never reduced modulo the order of the subgroup: this matters for
 * points outside the prime-order subgroup.
 * pm_jubjub_base: one point B with a device table of j 16^w B (w < 64, j = 1..8; 56 KiB), an opaque handle.
 *   _create: PM_ERR_BAD_ARG for a point off the curve, a coordinate >= r, NULL.  The table is built once, on the host.
 *   _from_key: the base of gadget `gadget_index` (the caller's index) of the key's current gadget table, which must be of kind
 *     PM_PLONK_GADGET_FIXED_BASE and whose table points t[0..R) as gathered by pm_plonk_key_set_gadgets (most significant round
 *     first: the order of dusk's gadget) must be curve points with t[k] = 2 t[k + 1]; the base is t[R - 1], the very point the
 *     gadget multiplies.  Anything else is PM_ERR_BAD_ARG.  Waits for the context's stream.  The handle does not refer to
 *     the key afterwards.
 *   _point: the point back (pure host; PM_ERR_BAD_ARG for NULL).  _free waits for the device before it releases the table.
 * The device calls take addresses on the context's GPU (16-byte aligned), NULL among them is PM_ERR_BAD_ARG, and launch
 * nothing for n = 0 (PM_OK); they run on `hip_stream` (NULL = the context's stream).
 *   pm_jubjub_fixed_mul_dev: out[i] = s_i B.  One kernel, no allocation; asynchronous.
 *   pm_jubjub_commit_dev: out[i] = v_i G + b_i H (a Pedersen commitment; g and h may be the same handle) in one pass over
 *     both scalars.  One kernel, no allocation; asynchronous.
 *   pm_jubjub_mul_dev: out[i] = s_i P_i.  d_out_xy == d_points_xy is allowed.  The points are NOT validated: for a point on
 *     the curve the law is complete; for any other input the output is unspecified, but the call does not fault (an
 *     inversion of 0 yields 0, as everywhere in this library).  The kernel is ordered on the stream like the others; the
 *     call allocates a window table for the threads in flight and releases it before it returns, which WAITS for the device.
 *   pm_jubjub_check_dev: *first_bad = the lowest index whose point is off the curve or has a coordinate >= r, n when every
 *     point passes.  WAITS for the stream.
 * The two host forms need no context and no GPU (csrc/host_field.h): plain double-and-add over the affine law, on purpose
 * another algorithm than the device's signed windows.  PM_ERR_BAD_ARG for a point off the curve, a coordinate or a scalar
 * >= r, an unknown scalar_form, NULL.
 * None of these calls is hardened against side channels: table addresses (device) and the sequence of additions (host)
 * depend on the scalar. */
typedef struct pm_jubjub_base pm_jubjub_base;
int pm_jubjub_base_create(pm_ctx* ctx, const uint64_t xy[8], pm_jubjub_base** out);
int pm_jubjub_base_from_key(pm_ctx* ctx, const pm_prover_key* key, size_t gadget_index, pm_jubjub_base** out);
int pm_jubjub_base_point(const pm_jubjub_base* base, uint64_t xy[8]);
void pm_jubjub_base_free(pm_ctx* ctx, pm_jubjub_base* base);
int pm_jubjub_fixed_mul_dev(pm_ctx* ctx, const pm_jubjub_base* base, const void* d_scalars, size_t n, uint32_t scalar_form,
                            void* d_out_xy, void* hip_stream);
int pm_jubjub_commit_dev(pm_ctx* ctx, const pm_jubjub_base* g, const pm_jubjub_base* h, const void* d_values,
                         const void* d_blinders, size_t n, uint32_t scalar_form, void* d_out_xy, void* hip_stream);
int pm_jubjub_mul_dev(pm_ctx* ctx, const void* d_points_xy, const void* d_scalars, size_t n, uint32_t scalar_form,
                      void* d_out_xy, void* hip_stream);
int pm_jubjub_check_dev(pm_ctx* ctx, const void* d_points_xy, size_t n, size_t* first_bad, void* hip_stream);
int pm_jubjub_mul_host(const uint64_t xy[8], const uint64_t scalar[4], uint32_t scalar_form, uint64_t out_xy[8]);
int pm_jubjub_add_host(const uint64_t p[8], const uint64_t q[8], uint64_t out_xy[8]);
/* ---- Native JubJub MSM: vector commitments ------------------------------------------------------------
 * pm_jubjub_msm_dev: out[b] = sum_i s_(b,i) P_i for `batch` >= 1 scalar vectors over the same n points: a Pedersen vector
 *   commitment per vector.  Vector b starts at element b * scalar_stride of d_scalars (scalar_stride >= n, elements of 32 bytes);
 *   d_out_xy receives `batch` affine points of 64 bytes, canonical Montgomery.  The multiplier of a point is the INTEGER
 *   0 <= s < r its scalar stands for, never reduced modulo l (the signed windows are an identity on integers), so points
 *   outside the prime-order subgroup are multiplied exactly.  n = 0 writes `batch` identities (0, 1).  The points are NOT
 *   validated (pm_jubjub_check_dev does that): for points on the curve the law is complete; for any other bytes, points or
 *   scalars (words >= r included), the output is unspecified but the call neither faults nor hangs -- every bucket index, count
 *   and cursor is bounded for any 256-bit pattern.
 *   The bucket method over signed c-bit windows, ceil(257 / c) of them (256 bits and the carry), 2^(c-1) buckets each; c follows
 *   from n by the rule of csrc/jubjub_msm_plan.h, or is forced with the option "jubjub_msm_window_bits" (4 .. 16; 0 = the
 *   rule; anything else PM_ERR_BAD_ARG).  The output BYTES do not depend on c, on the batch or on the order in which atomics
 *   land: the law is exact and the point leaves in affine form after one inversion.  Skewed scalars (all equal, all zero)
 *   are correct, only slower.
 *   Refusals: PM_ERR_BAD_ARG for NULL (points and scalars may be NULL when n = 0) or unaligned pointers, batch = 0,
 *   scalar_stride < n, a bad scalar_form, d_out_xy overlapping an input.  PM_ERR_LENGTH for what the plan cannot index:
 *   n > 2^31 - 1, scalar_stride > 2^40, n x windows x batch > 2^32 - 1 (digit, point) pairs, or windows x batch x 2^(c-1)
 *   > 2^28 buckets.  Asynchronous on `hip_stream` (NULL = the context's stream).  The workspace (4 bytes a pair, 144 a segment of 32
 *   pairs and 160 a bucket: 0.2 GB at 2^20 points) is cached in the context, ordered across streams, and given back by pm_trim.
 *   The floor: up to about 2^15 points the call is bound by latency (the doublings of one 256-bit chain, some 1.7 ms) exactly
 *   as pm_jubjub_mul_dev is, which is then as quick or up to 15 % quicker; the MSM wins from between 2^16 and 2^18 points on, 5 x at 2^20
 *   (DESIGN.md section 7.2m has the measurements).
 * pm_jubjub_msm_host: the plain sum of double-and-add products over the affine law, no context and no GPU: on purpose another
 *   algorithm than the device's.  PM_ERR_BAD_ARG for a point off the curve, a coordinate or scalar >= r, an unknown form, NULL
 *   (points and scalars may be NULL when n = 0). */
int pm_jubjub_msm_dev(pm_ctx* ctx, const void* d_points_xy, const void* d_scalars, size_t n, size_t scalar_stride, uint32_t batch,
                      uint32_t scalar_form, void* d_out_xy, void* hip_stream);
int pm_jubjub_msm_host(const uint64_t* points_xy, const uint64_t* scalars, size_t n, uint32_t scalar_form, uint64_t out_xy[8]);
/* ---- Native Schnorr signatures on JubJub: batch signing and verification ------------------------------
 * The check the VAR_BASE gadget exists for, outside a circuit: u G + c PK = R with c = H(R.x, R.y, m).  This is the SHAPE of
 * dusk-schnorr 0.7's single-key signature as remembered -- prior knowledge that nothing in this repository pins, exactly like
 * the sponge above and JUBJUB_GENERATOR: it is NOT claimed to produce dusk-schnorr's bytes.
 *   g         a pm_jubjub_base whose point has order exactly l = JUBJUB_ORDER, the order of the prime subgroup.  Checked on the
 *             host at the handle's first use here and remembered in the handle; PM_ERR_BAD_ARG, pm_last_error naming the cause,
 *             for the identity and for any point with l g != (0, 1).
 *   params    the Hades constants; capacity: the capacity word of pm_poseidon_hash_dev (canonical Montgomery).
 *   challenge h = the modelled sponge of pm_poseidon_hash_dev over the message (R.x, R.y, m): three elements, one chunk, so the
 *             sponge's padding 1 follows m.  c = the canonical integer of h with bits 250 and above cleared: c < 2^250 < l.
 *   sign      secret key sk and nonce k, integers in [0, r): R = k G (affine), u = (k - c sk) mod l.  A signature is
 *             (u, R.x, R.y): three 32-byte elements, 96 bytes.  The nonces are the CALLER's, as the blinders of
 *             pm_plonk_prove_zk are: the library has no random number generator, and a repeated or predictable nonce gives the
 *             key away.  sk = 0 or k = 0 modulo l are not refused.
 *   verify    public key PK = sk G, message m, signature (u, R) -> a reason, the LOWEST that applies:
 *               PM_SCHNORR_U_RANGE   u >= l (u + l would satisfy the equation as well)
 *               PM_SCHNORR_R_POINT   R is off the curve or has a coordinate >= r
 *               PM_SCHNORR_PK_POINT  the same for PK
 *               PM_SCHNORR_EQUATION  u G + c PK != R as points
 *               PM_SCHNORR_OK        none of them: valid
 *             The multipliers are exact integers, as everywhere in pm_jubjub_*; no cofactor is cleared, so a PK with a component
 *             of small order is judged exactly.
 * scalar_form (PM_SCALAR_MONTGOMERY or PM_SCALAR_CANONICAL, anything else is PM_ERR_BAD_ARG) governs sk, k and u, in and out.
 * Messages and coordinates are always canonical Montgomery elements; a message that is not below r is PM_ERR_BAD_ARG on the
 * host forms and gives an unspecified result, without a fault, on the device forms.
 * The device calls take addresses on the context's GPU (16-byte aligned; NULL among them is PM_ERR_BAD_ARG), run on
 * `hip_stream` (NULL = the context's stream) and launch nothing for n = 0 (PM_OK).
 *   pm_schnorr_sign_dev: n secret keys, nonces and messages (one element each) -> n signatures (three elements each) at d_sigs.
 *     One kernel, one thread a signature: k G over the base's window table, one inversion (R is hashed, so it must be affine),
 *     one permutation, the product modulo l.  Asynchronous, no allocation.  NOT hardened against side channels: the table
 *     addresses depend on k, and the arithmetic modulo l is not constant-time either.
 *   pm_schnorr_verify_dev: n public keys (two elements each), messages and signatures -> d_reasons, n uint32 (may be NULL), and
 *     *first_bad (may be NULL), the lowest index with a reason other than 0, n when every signature passes; with both NULL the
 *     call is PM_ERR_BAD_ARG.  No inversion: u G from the table, c PK by the signed 4-bit ladder of pm_jubjub_mul_dev over 63
 *     windows, then X = R.x Z and Y = R.y Z.  Two kernels on the stream (the tests, the hash and u G; then the ladder and the
 *     comparison), a pair per stride of the threads in flight.  The call allocates the ladder's window tables for those
 *     threads and releases them before it returns, which WAITS for the device, as pm_jubjub_mul_dev does; with first_bad it
 *     also waits for the stream.  A word of u that is not below r counts as u >= l in either form.
 * The two host forms need no context and no GPU (csrc/host_field.h): the affine law, double-and-add and long division modulo l,
 * on purpose other algorithms than the device's.  They take the base as a point and the Hades constants as
 * pm_hades_permute_host does, and return PM_ERR_BAD_ARG for what the device forms refuse, for constants _create refuses, and for
 * an sk, k, m or capacity that is not below r.  pm_schnorr_verify_host writes the reason; inputs it can judge are not errors. */
#define PM_SCHNORR_OK 0u
#define PM_SCHNORR_U_RANGE 1u
#define PM_SCHNORR_R_POINT 2u
#define PM_SCHNORR_PK_POINT 3u
#define PM_SCHNORR_EQUATION 4u
int pm_schnorr_sign_dev(pm_ctx* ctx, const pm_jubjub_base* g, const pm_hades_params* params, const uint64_t capacity[4],
                        const void* d_secret_keys, const void* d_nonces, const void* d_msgs, size_t n, uint32_t scalar_form,
                        void* d_sigs, void* hip_stream);
int pm_schnorr_verify_dev(pm_ctx* ctx, const pm_jubjub_base* g, const pm_hades_params* params, const uint64_t capacity[4],
                          const void* d_pks_xy, const void* d_msgs, const void* d_sigs, size_t n, uint32_t scalar_form,
                          void* d_reasons, size_t* first_bad, void* hip_stream);
int pm_schnorr_sign_host(const uint64_t g_xy[8], uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds,
                         uint32_t n_mds, const uint64_t capacity[4], const uint64_t sk[4], const uint64_t nonce[4],
                         const uint64_t msg[4], uint32_t scalar_form, uint64_t sig[12]);
int pm_schnorr_verify_host(const uint64_t g_xy[8], uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds,
                           uint32_t n_mds, const uint64_t capacity[4], const uint64_t pk_xy[8], const uint64_t msg[4],
                           const uint64_t sig[12], uint32_t scalar_form, uint32_t* reason);
/* pm_schnorr_verify_batch_dev: ONE equation for n signatures, a COFACTORED check.  With the caller's
 * weights z_i it computes W = a G + sum b_i PK_i - sum z_i R_i, a = sum z_i u_i mod l, b_i = z_i c_i mod l, by one
 * pm_jubjub_msm_dev over 2 n + 1 points, and accepts when 8 W = (0, 1).  The group has order 8 l, so the reductions modulo l
 * and the factor 8 belong together.
 *   d_weights  n integers 0 < z_i < 2^128, two uint64 each, little end first.  They are the CALLER's, as nonces and blinders are:
 *              the library has no random number generator.  A weight of 0 would drop its signature: PM_ERR_BAD_ARG, and
 *              pm_last_error names the lowest such index.
 *   d_sum_xy   NULL, or 64 bytes that receive W itself in affine form.
 *   *result, *first_bad (both required):
 *              some entry fails a structural test of pm_schnorr_verify_dev (u < l, R on the curve, PK on the curve): the lowest
 *                reason (PM_SCHNORR_U_RANGE / _R_POINT / _PK_POINT) of the lowest such index, and that index; such entries
 *                enter the sum as the identity, so W is still a curve point;
 *              all entries well formed and 8 W != (0, 1): PM_SCHNORR_EQUATION and n;
 *              accepted: PM_SCHNORR_OK and n.
 * What acceptance means.  A batch is accepted when every signature satisfies 8 (u G + c PK - R) = (0, 1); acceptance by the sum
 * implies this except with probability at most 2^-128 over weights drawn uniformly and independently of the signatures.  This is
 * WEAKER than pm_schnorr_verify_dev, which clears no cofactor: a signature its signer made with R = k G + T, T of small order,
 * fails there with PM_SCHNORR_EQUATION and passes here.  Every signature pm_schnorr_verify_dev accepts, this call accepts.
 * With predictable weights an attacker can make errors cancel.  On rejection, call pm_schnorr_verify_dev to find the culprit.
 * g must have order l: the same check and refusal as pm_schnorr_verify_dev; pointers are 16-byte aligned device addresses,
 * NULL among the inputs is PM_ERR_BAD_ARG unless n = 0 (accepted, W = (0, 1)); n > 2^30 - 1 is PM_ERR_LENGTH, as is what the
 * MSM's plan cannot index.  The call allocates the MSM's input (224 bytes a signature) and releases it, and it WAITS for the
 * stream, because it reads W back.  The floor: the batch wins from about 2^18 signatures on (2.4 x at 2^20); up to 2^12 the two
 * take the same time within 5 %, and between 2^14 and 2^16 pm_schnorr_verify_dev is up to 1.4 x quicker. */
int pm_schnorr_verify_batch_dev(pm_ctx* ctx, const pm_jubjub_base* g, const pm_hades_params* params, const uint64_t capacity[4],
                                const void* d_pks_xy, const void* d_msgs, const void* d_sigs, const void* d_weights, size_t n,
                                uint32_t scalar_form, void* d_sum_xy, uint32_t* result, size_t* first_bad, void* hip_stream);
/* ---- Poseidon cipher on JubJub keys: batch encryption, decryption and note scanning ------------------
 * Encrypting a note to its recipient, and the recipient's side: trial-decrypting every note of a ledger under one viewing key.
 * This is the SHAPE of dusk-poseidon's PoseidonCipher as remembered -- prior knowledge that nothing in this repository pins,
 * exactly like the sponge and the Schnorr signature above: it is NOT claimed to produce dusk-poseidon's bytes.
 *   P        the Hades permutation of `params` (width 5); L = msg_len, the message capacity, 1 .. 4 (dusk's is 2);
 *            S = (S.x, S.y) a JubJub point, the shared secret; init = [2^32, L, S.x, S.y, nonce].
 *   encrypt  s = P(init); for i < L: s[1 + i] += m[i], c[i] = s[1 + i]; s = P(s); c[L] = s[1].  A cipher is L + 1 elements.
 *   decrypt  s = P(init); for i < L: m[i] = c[i] - s[1 + i], s[1 + i] = c[i]; s = P(s); accepted when c[L] = s[1].
 *   a note   (R, nonce, c): the sender picks an ephemeral integer e, sends R = e G and encrypts under S = e PK, PK = vk G the
 *            recipient's key; the recipient holds the viewing key vk and recovers S = vk R.  Multipliers are the exact integers
 *            below r, as everywhere in pm_jubjub_*: no cofactor is cleared and nothing is reduced modulo l.
 * The status of a decryption is the LOWEST that applies:
 *   PM_CIPHER_OK     the tag matches
 *   PM_CIPHER_POINT  the secret (decrypt) or the ephemeral key R (scan) is off the curve or has a coordinate >= r
 *   PM_CIPHER_RANGE  the nonce or a cipher word is not below r
 *   PM_CIPHER_TAG    the tag does not match: not this key's note, or tampered with
 * For any status but PM_CIPHER_OK the L message words written are zero: the output bytes are deterministic and a wrong key's
 * garbage never leaves the device.
 * Elements and coordinates are canonical Montgomery, 32 bytes.  The device calls take addresses on the context's GPU (16-byte
 * aligned; NULL among the required ones is PM_ERR_BAD_ARG), run on `hip_stream` (NULL = the context's stream) and launch
 * nothing for n = 0 (PM_OK, *n_ok = 0).  msg_len outside 1 .. 4 is PM_ERR_BAD_ARG.  d_status receives n uint32 and may be NULL;
 * n_ok may be NULL, and with it the call WAITS for the stream and returns the count of status 0.  With both NULL, decrypt and
 * scan still write the messages, zero where refused.
 *   pm_poseidon_cipher_encrypt_dev: n secrets (two elements each), nonces and messages (L elements each) -> n ciphers (L + 1
 *     each).  One kernel, a thread a note, no allocation; asynchronous.  The secrets and messages are NOT validated: for
 *     anything that is not a curve point or not below r the output is unspecified, but the call does not fault (the rule of
 *     pm_jubjub_mul_dev).
 *   pm_poseidon_cipher_decrypt_dev: n secrets, nonces and ciphers -> n messages at d_msgs_out and their status.  One kernel;
 *     with n_ok it allocates the counter and releases it before it returns.
 *   pm_poseidon_cipher_scan_dev: n notes (ephemeral keys at d_ephemeral_xy, two elements each) under ONE viewing key, a host
 *     scalar in `scalar_form` (PM_SCALAR_MONTGOMERY or PM_SCALAR_CANONICAL, anything else is PM_ERR_BAD_ARG, as is a key that
 *     is not below r).  The 64 signed base-16 digits of vk are recoded once on the host and travel in the kernel's arguments:
 *     every thread multiplies by the same scalar, so a digit, its sign and the zero digit are wave-uniform.  Two kernels a
 *     stride of the threads in flight: the ladder vk R over the thread's own table 1 R .. 8 R with ONE inversion (S is hashed, so
 *     it must be affine), then the decryption with the curve test of R.  The call allocates the tables of those threads (1216
 *     bytes each) and releases them before it returns, which WAITS for the device, as pm_jubjub_mul_dev does.  R is not
 *     checked to lie in the prime-order subgroup.  NOT hardened against side channels: the table addresses depend on vk.
 *   pm_poseidon_cipher_scan_keys_dev: the same n notes under n_keys viewing keys, 1 ..
 *     PM_CIPHER_SCAN_MAX_KEYS of them, in one call.  view_keys: host, n_keys x 4 words in `scalar_form`; duplicates and a key of 0
 *     are legal.  With st_k[i] and m_k[i] the status and the message pm_poseidon_cipher_scan_dev gives note i under view_keys[k]:
 *       d_masks[i]    (required, n x uint64) bit k is set exactly when st_k[i] == PM_CIPHER_OK; bits n_keys and above are zero;
 *       d_status[i]   (n x uint32, 4-byte aligned, may be NULL) PM_CIPHER_POINT or PM_CIPHER_RANGE where the single-key scan
 *                     reports them -- both depend on the note alone --, else PM_CIPHER_OK when the mask is not zero, else
 *                     PM_CIPHER_TAG;
 *       d_msgs_out[i] (n x L elements, may be NULL) m_k[i] for the LOWEST set k, zeros when the mask is zero.  Only the lowest
 *                     key's message is returned: two keys open one note only when they give the same S (duplicate keys, R the
 *                     identity, keys that agree modulo the order of R), and then they give the same message;
 *       *n_hits       (may be NULL) the set bits over all masks; with it the call WAITS for the stream, as n_ok does.
 *     PM_ERR_BAD_ARG before a byte changes for n_keys outside 1 .. 64, a key not below r, a bad scalar_form or msg_len, a NULL
 *     or misaligned required pointer.  n = 0 launches nothing: PM_OK, *n_hits = 0.  From "cipher_scan_keys_table_min" keys on
 *     (pm_set_option) the call builds, once per note, the full window table e 16^w R (w = 0 .. 63, e = 1 .. 8; 73 728 bytes a
 *     note in flight) and every key then costs at most 64 additions and one inversion, no doubling; below it the single-key
 *     ladder runs per key.  Either path writes the same bytes, and they depend neither on the scratch budget nor on the stream: S
 *     is brought to its canonical affine form before it is hashed.  The call allocates pm_poseidon_cipher_scan_keys_work_bytes
 *     of scratch (PM_ERR_OOM with no output byte written when that fails) and releases them before it returns, which WAITS for
 *     the device.  The option "cipher_scan_table_mb" caps that scratch: the notes in flight are the largest multiple of 64
 *     that fits, at least 64; 0 = no cap.  No more hardened against side channels than pm_poseidon_cipher_scan_dev.
 * The two host forms need no context and no GPU (csrc/host_field.h) and take the Hades constants as pm_hades_permute_host does.
 * PM_ERR_BAD_ARG for constants _create refuses, msg_len outside 1 .. 4, NULL, and on encrypt for a secret off the curve or a
 * word that is not below r.  pm_poseidon_cipher_decrypt_host writes the status; inputs it can judge are not errors. */
#define PM_CIPHER_OK 0u
#define PM_CIPHER_POINT 1u
#define PM_CIPHER_RANGE 2u
#define PM_CIPHER_TAG 3u
int pm_poseidon_cipher_encrypt_dev(pm_ctx* ctx, const pm_hades_params* params, const void* d_secrets_xy, const void* d_nonces,
                                   const void* d_msgs, uint32_t msg_len, size_t n, void* d_ciphers, void* hip_stream);
int pm_poseidon_cipher_decrypt_dev(pm_ctx* ctx, const pm_hades_params* params, const void* d_secrets_xy, const void* d_nonces,
                                   const void* d_ciphers, uint32_t msg_len, size_t n, void* d_msgs_out, void* d_status,
                                   size_t* n_ok, void* hip_stream);
int pm_poseidon_cipher_scan_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t view_key[4], uint32_t scalar_form,
                                const void* d_ephemeral_xy, const void* d_nonces, const void* d_ciphers, uint32_t msg_len, size_t n,
                                void* d_msgs_out, void* d_status, size_t* n_ok, void* hip_stream);
#define PM_CIPHER_SCAN_MAX_KEYS 64u
int pm_poseidon_cipher_scan_keys_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t* view_keys, uint32_t n_keys,
                                     uint32_t scalar_form, const void* d_ephemeral_xy, const void* d_nonces, const void* d_ciphers,
                                     uint32_t msg_len, size_t n, void* d_masks, void* d_msgs_out, void* d_status, size_t* n_hits,
                                     void* hip_stream);
/* the scratch that call allocates under the context's options; 0 for arguments it refuses and for n = 0 */
size_t pm_poseidon_cipher_scan_keys_work_bytes(pm_ctx* ctx, uint32_t n_keys, uint32_t msg_len, size_t n);
int pm_poseidon_cipher_encrypt_host(uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds,
                                    const uint64_t secret_xy[8], const uint64_t nonce[4], const uint64_t* msg, uint32_t msg_len,
                                    uint64_t* cipher_out);
int pm_poseidon_cipher_decrypt_host(uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds,
                                    const uint64_t secret_xy[8], const uint64_t nonce[4], const uint64_t* cipher, uint32_t msg_len,
                                    uint64_t* msg_out, uint32_t* status);
/* ---- JubJub wire format: batch point decoding with square roots in Fr on the GPU --------------------
 * A ledger keeps a JubJub point -- the ephemeral key of a note, a public key, the R of a signature -- as 32 bytes: the canonical
 * y, little-endian, with the least significant bit of the canonical x in bit 7 of byte 31.  This is the SHAPE of
 * JubJubAffine::to_bytes / from_bytes as remembered -- prior knowledge that nothing in this repository pins, exactly like the
 * cipher and the Schnorr signature above: it is NOT claimed to accept dusk-jubjub's bytes.  One decision is stricter than the
 * 2019-era from_bytes as remembered: x = 0 with the sign bit set is REFUSED, so the accepted bytes are exactly the image of the
 * encoder and decode-then-encode is the identity.
 *
 * Square roots.  pm_fr_sqrt_dev: n canonical Montgomery elements at d_in -> n roots at d_out (d_out == d_in is allowed) and n
 * uint32 flags at d_is_square (may be NULL): 1 and the root whose canonical integer is EVEN (0 for 0) for a square, 0 and root 0
 * for a non-square or an input that is not below r.  One thread an element, no data-dependent trip count: one fixed
 * exponentiation, the discrete logarithm in the subgroup of order 2^32 by four 8-bit windows against tables the context builds
 * once (49 KiB of device memory, released by pm_trim and at shutdown).  n_square may be NULL; with it the call WAITS for the
 * stream and returns the count of flag 1.  pm_fr_sqrt_host: one element on the CPU, no context, by the plain Tonelli-Shanks
 * loop: on purpose another algorithm.
 *
 * Decoding: clear the sign bit and require y < r; x = sqrt((y^2 - 1) / (1 + d y^2)) (the denominator is never zero: -1 / d is
 * a non-square), negated when its parity differs from the sign bit.  The status of a point is the LOWEST that applies:
 *   PM_JUBJUB_OK                   decoded
 *   PM_JUBJUB_BAD_RANGE            y (bits 0 .. 254) is not below r
 *   PM_JUBJUB_BAD_NOT_ON_CURVE     (y^2 - 1) / (1 + d y^2) is not a square: no point has this y
 *   PM_JUBJUB_BAD_SIGN             x = 0 with the sign bit set
 *   PM_JUBJUB_BAD_NOT_IN_SUBGROUP  only with PM_JUBJUB_CHECK_SUBGROUP: [l] P is not the identity (the identity passes)
 * A refused point is written as (0, 0), which is off the curve, so every later call refuses it: a scan answers PM_CIPHER_POINT,
 * a verification its bad-R / bad-PK reason.  A refused point is NOT an error of the call: a ledger holds other people's
 * garbage, so the verdict is per point, as in the cipher calls.  PM_JUBJUB_CHECK_SUBGROUP is OFF by default because it costs a
 * whole 256-doubling ladder a point (the wave-uniform ladder of the scan under the digits of l, with a table of 1152 bytes a
 * thread in flight that the call allocates and releases, which WAITS for the device) where the decoding itself is a few
 * hundred products.
 *   pm_jubjub_decompress_dev: record i is the 32 bytes at d_bytes + i in_stride_bytes; point i (x | y, canonical Montgomery)
 *     goes to d_out_xy + i out_stride_bytes.  A stride of 0 means packed (32 and 64 bytes); otherwise it is a multiple of 16
 *     that is at least the packed size, anything else is PM_ERR_BAD_ARG, as are unknown flag bits, NULL among the required
 *     pointers and a pointer that is not 16-byte aligned.  A strided call touches nothing between its records: the R halves
 *     of n signatures (u | R, 64 bytes) decode with in_stride_bytes = 64, out_stride_bytes = 96 straight into (u, R.x, R.y)
 *     records.  Input and output must not overlap.  d_status receives n uint32 and may be NULL; n_ok may be NULL, and with it
 *     the call WAITS for the stream and returns the count of status 0.  n = 0 launches nothing (PM_OK, *n_ok = 0).
 *   pm_jubjub_compress_dev: n points (64 bytes each, packed) -> n x 32 bytes at d_bytes_out, which must not overlap them.  The
 *     points are NOT validated (the rule of pm_jubjub_mul_dev): anything that is not a canonical point gives unspecified
 *     bytes, but the call does not fault.  Asynchronous.
 *   pm_dev_copy_strided: `rows` runs of width_bytes from d_src + i src_stride_bytes to d_dst + i dst_stride_bytes, device to
 *     device on hip_stream, asynchronous: how the u halves of byte signatures reach their records.  Strides are at least the
 *     width; rows = 0 or width_bytes = 0 copies nothing.
 * The host forms need no context and no GPU (csrc/host_field.h).  pm_jubjub_decompress writes the status; bytes it can judge
 * are not errors.  pm_jubjub_compress returns PM_ERR_BAD_ARG for a point off the curve or a coordinate that is not below r. */
#define PM_JUBJUB_CHECK_SUBGROUP 1u
#define PM_JUBJUB_OK 0u
#define PM_JUBJUB_BAD_RANGE 1u
#define PM_JUBJUB_BAD_NOT_ON_CURVE 2u
#define PM_JUBJUB_BAD_SIGN 3u
#define PM_JUBJUB_BAD_NOT_IN_SUBGROUP 4u
int pm_fr_sqrt_dev(pm_ctx* ctx, const void* d_in, size_t n, void* d_out, void* d_is_square, size_t* n_square, void* hip_stream);
int pm_fr_sqrt_host(const uint64_t a[4], uint64_t out[4], uint32_t* is_square);
int pm_jubjub_compress(const uint64_t xy[8], uint8_t out[32]);
int pm_jubjub_decompress(const uint8_t in[32], uint32_t flags, uint64_t xy[8], uint32_t* status);
int pm_jubjub_compress_dev(pm_ctx* ctx, const void* d_xy, size_t n, void* d_bytes_out, void* hip_stream);
int pm_jubjub_decompress_dev(pm_ctx* ctx, const void* d_bytes, size_t in_stride_bytes, size_t n, uint32_t flags, void* d_out_xy,
                             size_t out_stride_bytes, void* d_status, size_t* n_ok, void* hip_stream);
int pm_dev_copy_strided(pm_ctx* ctx, void* d_dst, size_t dst_stride_bytes, const void* d_src, size_t src_stride_bytes,
                        size_t width_bytes, size_t rows, void* hip_stream);
/* Proof::to_bytes: 11 x 48-byte compressed G1, then the 16 scalars of ProofEvaluations::to_bytes. */
int pm_plonk_proof_to_bytes(const pm_plonk_proof* proof, uint8_t out[PM_PLONK_PROOF_BYTES]);
/* ---- The prover with coefficient-range ownership end to end (SURVEY.md section 8e row 3 + 8f N5; configs[4]) ----------
 * pm_plonk_prove_sharded splits only the MSMs: every rank still holds every polynomial and repeats every transform.
 * Here rank r of `world` (a power of two, world^2 <= n) owns rows / coefficients [r n / world, (r + 1) n / world) of
 * every vector and nothing else -- workspace / world, no replicated transform: the size-n transforms run as
 * pm_fr_ntt_fourstep_batch_dev over the ranks (all the polynomials of a round in one sequence of all-to-alls), the 4n-coset
 * work as four size-n sub-coset transforms whose results stay in the block-transposed order (the quotient is pointwise; its
 * one next-row access reads the halo row the transform delivers), and prefix product, openings and Ruffini division are
 * local passes plus one all-gather of per-rank scalars each: 12 all-to-all calls and 8 all-gathers per proof
 * (pm_comm_stats).  The proof and the verifier key are bit-identical to pm_plonk_prove's on every rank.
 *   allgather: gathers ONE fixed-size message per rank (PM_COMM_MSG_WORDS u64 words, host memory; word 0 = a count,
 *              0 = the abort marker of a rank that gave up) into gathered[world][PM_COMM_MSG_WORDS]; returns 0 on success.
 *              NULL = the context's RCCL communicator (pm_comm_init).  8 per proof (the first an agreement on the
 *              arguments: public inputs, flags and size must be the same on every rank), 2 + 2 per key.
 *   alltoall:  the callback of pm_fr_ntt_fourstep_dev (device buffers); NULL = the communicator.
 * Inputs are the rank's slices: selector_slices[s] = m = n / world rows of selector s (NULL = identically zero on this
 * rank), sigma_index_slices = [4][m] (wire j of row rank m + i is followed by position sigma_index, a GLOBAL index
 * j' n + i'), commit_key_slice = powers [rank m, (rank + 1) m) of the commit key, d_witness_slices = [4][m] wire values
 * in device memory.  Public inputs are passed whole (positions are global) on every rank.  A rank whose arguments are
 * bad meets its peers in the agreement all-gather with the abort marker: every rank returns an error, nobody blocks.  A
 * rank that fails later (a HIP error between two all-to-alls) returns its error and sends the marker to the next
 * all-gather, but an all-to-all has no marker and no timeout: treat such an error as fatal for the group.
 * pm_plonk_dist_key_bytes: device memory this rank holds for the key and its per-proof workspace. */
#define PM_COMM_MSG_WORDS 289   /* 1 + 18 x PM_COMM_MAX_POINTS */
typedef int (*pm_allgather_fn)(void* user, const uint64_t* msg, uint64_t* gathered);
typedef struct pm_dist {
  uint32_t world, rank;
  pm_allgather_fn allgather;
  pm_alltoall_fn alltoall;
  void* user;
} pm_dist;
typedef struct pm_dist_key pm_dist_key;
int pm_plonk_preprocess_dist(pm_ctx* ctx, const pm_dist* dist, const uint64_t* const selector_slices[PM_PLONK_SELECTORS],
                             const int64_t* sigma_index_slices, size_t n, pm_dist_key** out);
void pm_plonk_dist_key_free(pm_ctx* ctx, pm_dist_key* key);
size_t pm_plonk_dist_key_bytes(const pm_dist_key* key);
int pm_plonk_key_commit_dist(pm_ctx* ctx, const pm_dist* dist, pm_dist_key* key, const pm_bases* commit_key_slice,
                             const char* transcript_label, uint64_t (*verifier_key_out)[12]);
int pm_plonk_prove_dist(pm_ctx* ctx, const pm_dist* dist, pm_dist_key* key, const pm_bases* commit_key_slice,
                        const void* d_witness_slices, const uint64_t* pi_positions, const uint64_t* pi_values, size_t n_pi,
                        uint32_t flags, pm_plonk_proof* out);

/* Every label string of the transcript, in message order, as "key=label" lines (a static string).  The labels are
 * restated from the published dusk-plonk 0.8 design and are PARITY-UNPINNED; they live in ONE table (csrc/prover_transcript.h,
 * namespace tl) that both the native prover and the Python verifier side read -- the single place to edit when
 * upstream vectors become available. */
const char* pm_plonk_transcript_labels(void);
/* The same with the SRS split over the GPUs of a node (BASELINE.json configs[4]): every rank calls this with
 * the same witness and its own slice of the commit key -- bases for coefficients [first_coefficient,
 * first_coefficient + pm_g1_bases_len(slice)) -- and `exchange` turns this rank's k partial points (k x 18
 * limbs, in place) into the sums over all ranks: an all-gather of k x 144 bytes followed by pm_g1_fold per
 * point.  exchange = NULL uses the context's RCCL communicator (pm_comm_init).  A callback is also entered
 * with k = 0 when this rank's local work failed: it must tell the peers (so that none blocks) and return
 * non-zero; a non-zero return aborts with PM_ERR_EXCHANGE. */
typedef int (*pm_exchange_fn)(void* user, uint64_t* xyz, uint32_t k);
int pm_plonk_key_commit_sharded(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key_slice,
                                size_t first_coefficient, pm_exchange_fn exchange, void* user,
                                const char* transcript_label, uint64_t (*verifier_key_out)[12]);
int pm_plonk_prove_sharded(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key_slice, size_t first_coefficient,
                           const void* d_witness, const uint64_t* pi_positions, const uint64_t* pi_values, size_t n_pi,
                           uint32_t flags, pm_exchange_fn exchange, void* user, pm_plonk_proof* out);

/* ---- the exchange step inside the library (SURVEY.md sections 8b, 8e) ------------------------------- */
/* One process per GPU, one pm_ctx per process.  Rank 0 makes the id and hands its 128 bytes to the other ranks
 * out of band (MPI, a file, the host runtime's own broadcast); every rank then calls pm_comm_init, which is
 * collective (ncclCommInitRank over xGMI).  RCCL is bound at run time (dlopen of librccl.so.1).
 * pm_g1_allgather_fold: every rank passes its k <= PM_COMM_MAX_POINTS partial points (k x 18 limbs,
 * projective); on return each holds the sums over all ranks -- one ncclAllGather of a fixed 2312-byte message
 * per rank, then pm_g1_fold per point: an all-reduce under the group law (RCCL has no such reduction).  k = 0
 * is the abort marker of a rank whose local work failed: it still takes part, and the call returns
 * PM_ERR_EXCHANGE on every rank instead of leaving the peers blocked. */
#define PM_COMM_ID_BYTES 128
#define PM_COMM_MAX_POINTS 16
int pm_comm_unique_id(uint8_t id[PM_COMM_ID_BYTES]);
int pm_comm_init(pm_ctx* ctx, const uint8_t id[PM_COMM_ID_BYTES], int rank, int world);
int pm_comm_destroy(pm_ctx* ctx);
int pm_comm_info(const pm_ctx* ctx, int* rank, int* world);
int pm_g1_allgather_fold(pm_ctx* ctx, uint64_t* xyz, uint32_t k);
/* test hook: the fold step on `world` messages of 1 + 16 x 18 words ([count | points]) given by the caller */
int pm_test_fold_gathered(const uint64_t* msgs, int world, uint32_t k, uint64_t* out_xyz);
/* A dead peer INSIDE an exchange: pm_set_option(ctx, "comm_timeout_ms", T) with T > 0 (default 0 = off) puts every exchange
 * on the context's communicator -- the message all-gather and the all-to-all of the rank-split transform -- under a
 * deadline that covers both the enqueue and the wait for its completion (with the option on, an all-to-all is waited
 * for where it is issued).  When T ms pass without completion the context's watch thread calls ncclCommAbort, the
 * blocked call returns, the entry point returns PM_ERR_EXCHANGE (pm_last_error names the exchange and the option) and
 * the communicator is DEAD: every later exchange on it returns PM_ERR_EXCHANGE at once, until pm_comm_destroy +
 * pm_comm_init on every rank.  Choose T well above the slowest legitimate exchange (the peers of a 2^24-gate proof
 * arrive at their all-gathers tens of milliseconds apart; a first all-to-all also sets up connections).  The callback
 * transports have their own containment (a broken barrier).  Test hook, no GPU and no RCCL: the same deadline logic on a
 * stub table whose all-gather blocks until its communicator is aborted (peer_answers = 0) or returns at once (1):
 * first_rc / second_rc = two exchanges in a row, elapsed_ms = the first one's duration, aborts = ncclCommAbort calls. */
int pm_test_comm_deadline(long timeout_ms, int peer_answers, int* first_rc, long* elapsed_ms, int* second_rc, int* aborts,
                          char* err_out, size_t err_cap);

/* Keccak-f[1600] on a 200-byte state (host; the permutation under the Merlin / STROBE-128 transcript
 * the prover derives its challenges from -- merlin is a dependency of dusk-plonk, ref:Cargo.toml:19). */
void pm_keccak_f1600(uint8_t state[200]);

/* ---- introspection / tuning (not needed by the prover) --------------------------------- */

/* Number of kernel launches and the Stockham radices the library will use for 2^log_n. */
int pm_ntt_plan(uint32_t log_n, uint32_t radix_log2[4], uint32_t* n_passes);
/* Override tunables: "msm_window_bits", "jubjub_msm_window_bits" (pm_jubjub_msm_dev: 4 .. 16, 0 = the rule), "msm_chunk", "msm_lb", "msm_max_pairs", "msm_pipeline" (1 = a batched MSM as
 * pipelined pieces on two streams; off: it measured slower), "ntt_tile_log", "ntt_radix", "ntt_max_radix", "ntt_xcd",
 * "ntt_direct_tw", "ntt_tw_producer" (1, the default: the radix-4 first pass of radix 2^10 multiplies its outputs by the next
 * pass's inter-pass twiddle table, so that pass starts on its data alone; 0: every pass multiplies its own inputs.  Same results either way;
 * it needs "ntt_direct_tw" = 1), "ntt_step_prio" (1, the default: the waves of a radix-4 pass of radix 2^10 lower their issue priority step by
 * step, so that the two workgroups of a CU alternate instead of one running ahead; 0: age alone.  Same results either way; any other
 * value is PM_ERR_BAD_ARG), "ntt_fixed_shape" (2, the default: a pass launch whose size, place in the plan, flags and layout are exactly
 * those of a fixed-shape kernel takes that kernel, which has the geometry and the flags compiled in: both radix-2^10 passes of a plain 2^20
 * transform, forward or inverse, batched or not; 1: the first pass of that transform only, the last one takes the generic kernel;
 * 0: every launch takes the generic kernel.  Same results in all three; any other value is PM_ERR_BAD_ARG), "ntt_pipeline" (0 = no copy / compute overlap in pm_fr_ntt_batch), "poly_lookback" (prefix product in one
 * pass: 0 never, 1 while all tiles are resident -- the default --, 2 always).  PM_ERR_BAD_ARG if unknown. */
int pm_set_option(pm_ctx* ctx, const char* key, long value);
/* Opt-in per-kernel timing with hipEvents recorded on the launch stream (bench.py's roofline
 * leg).  pm_profile_read writes lines "<kernel> <launches> <total_ms>\n" into buf. */
int pm_profile_enable(pm_ctx* ctx, int on);
/* Restrict the timers to one kernel name (as printed by pm_profile_read), NULL = all: an event pair
 * costs ~5 us of launch stream time, so a timed region that needs one kernel's duration asks for that one. */
int pm_profile_select(pm_ctx* ctx, const char* kernel_name);
int pm_profile_read(pm_ctx* ctx, char* buf, size_t cap);
/* Elementwise field kernels used by the parity tests: op 0 = Fr mul, 1 = Fr add, 2 = Fr sub,
 * 3 = Fp mul, 4 = Fp add, 5 = Fp sub, 6 = Fr inverse of a, 7 = Fp inverse of a (b ignored, may be NULL; 0 -> 0).  Host pointers,
 * n elements. */
int pm_test_field_op(pm_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out,
                     size_t n);
/* The shared inline device routines on RAW limbs (csrc/test_hooks.hip): operands are radix-2^W limbs as given (field 0 = Fr:
 * 9 x 29 bit, 1 = Fp: 14 x 28 bit; one uint32 per limb, no unpacking, no reduction) and the result limbs come back as the
 * routine left them (no canonical packing).  One thread per case; a case is IN elements in, OUT elements out, back to back.
 * op (IN -> OUT): 0 fe_add (2 -> 1), 1 fe_norm, 2 fe_norm_full (1 -> 1), 3 fe_mul (2 -> 1), 4 fe_sqr (1 -> 1), 5 fe_mul_limb
 * (a, b0 in limb 0 of the second: 2 -> 1), 6 fe_mul2 (a0 b0 a1 b1: 4 -> 2), 7 fe_mul3 (6 -> 3), 8 fe_mma2 (a0 b0 c0 d0 a1 b1:
 * 6 -> 2), 9 fe_sqr2 (2 -> 2), 10 fe_reduce_weak, 11 fe_unpack (NS saturated words in the first limbs), 12 fe_canon_pack (NS
 * saturated words out, then zeros), 13 fe_pow2 (limb 0 selects the exponent: 0 = W N, 1 = 2 W N - 32 NS, 2 = 64 NS + W N)
 * (1 -> 1 each), 14 fe_mul_split<5,6> (x, 2 rows: 3 -> 1), 15 fe_mul_split<1,2> (x, 9 rows: 10 -> 1) (Fr), 16
 * fp_is_zero_product, 17 fp_is_zero_lazy (1 -> 1, 0 / 1 in limb 0) (Fp), 18 dft8 (x[0..7], w1, w2, w3: 11 -> 8), 19 dft4
 * (a0..a3, w4: 5 -> 4) (Fr), 20 fe_canon_limbs, 21 fe_inv_int, 22 fe_inv_dev (csrc/field_inv.hip.h; 1 -> 1; cases 64 k ..
 * 64 k + 63 share a wave, whose vote ends the rounds of fe_inv_int), 32 + K fe_sub<K,1> (2 -> 1) for the K the library
 * instantiates (Fr 2, 3, 5, 9, 18, 34, 39; Fp 2, 3, 5, 6, 8, 11), 24 fe_reduce_canon_pack (1 -> 1, a wave per 64 cases), the
 * lazy split products (D = G: limbs normalised, value up to 16.01 r / 37.01 r / 11.01 r) 25 fe_mul_split<3,3> (x, 3 rows:
 * 4 -> 1), 26 fe_mul_split<1,1> (x, 9 rows: 10 -> 1), 27 fe_mul_split<5,5> (x, 2 rows: 3 -> 1) (Fr).  PM_ERR_BAD_ARG for any other (field, op).  Host pointers, n cases. */
int pm_test_field_raw_op(pm_ctx* ctx, int field, int op, const uint32_t* in, uint32_t* out, size_t n);
/* The XYZZ group law of csrc/ec.hip.h on raw limbs.  A point is 57 words: X, Y, ZZ, ZZZ (14 Fp limbs each), infinity flag.
 * op 0 = xyzz_double_affine (X, Y of a), 1 = xyzz_double, 2 = xyzz_madd (X, Y of b: the affine operand), 3 = xyzz_add, 4 =
 * xyzz_mul_small (word 0 of b: the multiplier), 5 = half_double, 6 = half_add (one point per lane pair, as the reduction
 * kernels hold it).  b may be NULL for the doublings.  An infinite result has all limbs zero.  Host pointers, n cases. */
int pm_test_g1_raw_op(pm_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n);
/* The GLV split of csrc/ec_mul.hip.h, k = k1 + k2 z^2 with z^2 = 0xac45a4010001a4020000000100000000, on the device as the
 * kernels run it: n scalars (host pointer, n x 32 bytes, either PM_SCALAR_* form, below r) -> out, n x {k1 lo, k1 hi, k2
 * lo, k2 hi} as uint64. */
int pm_test_glv_split(pm_ctx* ctx, const uint64_t* scalars, size_t n, uint32_t scalar_form, uint64_t* out);
/* Pure host, no context: the same routine compiled for the host, on one canonical k < r. */
int pm_test_host_glv_split(const uint64_t k[4], uint64_t out[4]);
/* The arithmetic modulo l = JUBJUB_ORDER behind the Schnorr calls (csrc/jubjub_scalar.hip.h), one thread a case: plain integers
 * of four uint64 in and out, host pointers, n cases.  op 0 = a mod l (a < r; b and c are not read and may be NULL), 1 =
 * (a - b c) mod l (a, b < r, c < 2^250), 2 = a < l as 0 / 1 in word 0 (the other words zero).  PM_ERR_BAD_ARG for another op. */
int pm_test_jubjub_scalar_op(pm_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, size_t n);
/* Pure host, no context: the same three operations by the host's long division (csrc/host_field.h), for any four-word operands. */
int pm_test_host_jubjub_scalar_op(int op, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, size_t n);
/* Signatures pm_schnorr_verify_dev has in flight at once on this context's GPU: beyond it the kernel walks n in strides. */
int pm_test_schnorr_stride(pm_ctx* ctx, size_t* stride);
/* Notes pm_poseidon_cipher_scan_dev has in flight at once on this context's GPU: beyond it the call walks n in strides. */
int pm_test_cipher_stride(pm_ctx* ctx, size_t* stride);
/* Pure host, no context: the recoding of a viewing key that pm_poseidon_cipher_scan_dev passes to its kernel, 64 signed base-16
 * digits with the TOP one first: digits[k] = d_(63 - k), sum d_w 16^w = the integer of the key, every |d_w| <= 8.
 * PM_ERR_BAD_ARG for a key that is not below r, an unknown scalar_form, NULL. */
int pm_test_cipher_digits(const uint64_t view_key[4], uint32_t scalar_form, int8_t digits[64]);
/* Pure host, no context: the plan of pm_poseidon_cipher_scan_keys_dev on its full-table path (csrc/cipher_scan_plan.h) for a
 * GPU of num_cus CUs and the budget table_mb of the option "cipher_scan_table_mb" (0 = no cap): the notes in flight, a multiple
 * of 64 between 64 and num_cus x 8 x 64 and no more than n rounded up to 64, and the scratch bytes = stride x (73 728 +
 * n_keys x (64 + 32 msg_len)) + 64 n_keys + 16.  n = 0 gives 0 and 0.  PM_ERR_BAD_ARG for n_keys outside 1 .. 64, msg_len
 * outside 1 .. 4, a negative budget, NULL. */
int pm_test_cipher_scan_keys_plan(uint32_t num_cus, uint32_t n_keys, uint32_t msg_len, size_t n, long table_mb, size_t* stride,
                                  size_t* bytes);
/* Pure host, no context: the plan of pm_jubjub_msm_dev for n points and `batch` vectors (csrc/jubjub_msm_plan.h); window_bits as
 * the option "jubjub_msm_window_bits" (0 = the rule); num_cus is accepted for symmetry with the other plan hooks and not used:
 * this plan does not depend on the machine.  out[8] = {0 window bits c, 1 windows of a scalar = ceil(257 / c), 2 buckets per
 * window = 2^(c-1), 3 (digit, point) pairs at most = n x windows x batch, 4 workspace bytes, 5 bucket sets = windows x batch,
 * 6 segments at most (accumulate threads), 7 buckets per thread of the window kernel}.  Returns what the call would:
 * PM_ERR_BAD_ARG (batch = 0, a width outside 4 .. 16), PM_ERR_LENGTH (the limits of pm_jubjub_msm_dev); out is then zero. */
int pm_test_jubjub_msm_plan(size_t n, uint32_t batch, long window_bits, uint32_t num_cus, uint64_t out[8]);
/* Pure host, no context: what pm_poseidon_ledger_append_dev launches when k leaves are appended to a tree of `height` that
 * holds `count` (the plan the call itself runs from).  For level l = 1..height, at index l - 1 of three arrays of `height`
 * entries each: first[] = the first node hashed, nodes[] = their number, below[] = the stored width of level l - 1 after the
 * append.  *chain_from = the first level whose range is one node (every level from there on has one), *hashed = the sum
 * of nodes[].  k = 0: every entry 0, *chain_from = 0.  Any output may be NULL.  PM_ERR_BAD_ARG for a height outside 1 .. 31 or
 * count > 4^height, PM_ERR_LENGTH for count + k > 4^height or k > 2^31 - 1. */
int pm_test_ledger_plan(uint32_t height, uint64_t count, uint64_t k, uint64_t* first, uint64_t* nodes, uint64_t* below,
                        uint32_t* chain_from, uint64_t* hashed);
/* Pure host, no context: the signed-window recoding the kernels run, compiled for the host, on ANY 256-bit integer (four words,
 * little end first) at width c in 4 .. 16 (else PM_ERR_BAD_ARG): digits[k], k < *n_digits, with sum digits[k] 2^(c k) = the
 * integer and |digits[k]| <= 2^(c-1).  *n_digits is the plan's window count; a carry out of the top window would show as one
 * more digit (it never occurs).  digits must hold 66 entries. */
int pm_test_jubjub_msm_digits(const uint64_t scalar[4], uint32_t c, int32_t* digits, uint32_t* n_digits);
/* Pure host, no context: the host-side field arithmetic behind the MSM fold and the prover's challenge scalars
 * (csrc/host_field.h).  op 0 = Fr product, 1 = Fp product, 2 = Fr inverse (binary extended Euclid), 3 = Fp inverse, 4 / 5 =
 * the same inverses by exponentiation; Montgomery form in and out, n elements; b is ignored by the inversions. */
int pm_test_host_field_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* Pure host, no device: the library's sizing pass for one MSM piece of this shape -- out[4] = {its return code, device
 * workspace bytes, pinned host bytes, (digit, point) pairs at most}. */
int pm_test_msm_sizing(size_t n, uint32_t batch, long window_bits, uint32_t table_window_bits, uint32_t num_cus,
                       uint64_t out[4]);
/* Pure host, no device: the decisions of that plan (csrc/msm_plan.h), with the options "msm_chunk" / "msm_lb" as chunk /
 * lb (0 = the library's choice; num_cus 0 = 256) -- out[32] = {0 the plan's return code, 1 window bits, 2 bucket sets of
 * the piece, 3 level-1 chunk, 4 shortest chunk for sparse inputs, 5 chunk handed to the histogram kernel, 6 accumulate
 * levels, 7 level-1 threads, 8 level-1 workgroups, 9 threads per level-1 workgroup, 10 level-1 placement request (LDS
 * bytes: 82944, 55296 or 0), 11 buckets per lane pair in the bucket reduction (lb), 12 log2 lb, 13 level-1 waves per set
 * (n1), 14 follow-up reduction levels (n_dev), 15-17 their groups per set, 18 items per set left for the fold, 19
 * sequences the fold receives, 20 bit planes among them, 21 the device applies the weights (1) or the host fold does (0),
 * 22 tiles per histogram workgroup, 23 histogram workgroups per MSM, 24 scatter workgroups, 25 partitions, 26-31 zero}.
 * level_len (may be NULL, 8 entries): entries read by each accumulate level, saturated to 32 bits, zero past the last. */
int pm_test_msm_plan(size_t n, uint32_t batch, long window_bits, uint32_t table_window_bits, uint32_t num_cus, long chunk,
                     long lb, uint32_t out[32], uint32_t* level_len);
/* Pure host, no context: the pass plan of a transform of 2^log_n points (tunables 0 = a fresh context's defaults) --
 * out[20] = {passes, 4 x {log2 radix, log2 columns per tile, threads per workgroup, LDS bytes}, mask of passes that have
 * a kernel, log2 group size of the blocked intermediate layout, 0}. */
int pm_test_ntt_plan(uint32_t log_n, uint32_t batch, long tile_log, long max_radix, long radix, uint32_t num_cus,
                     uint32_t out[20]);
/* The radix-4 step table of radix 2^S (2 <= S <= 10) of one direction as the pass kernels read it, built on first use:
 * seven head constants of 84 words (w4, then w16^e for e = 1, 2, 3, 6, 9, 0; word 9 b + j = limb b of w 2^(29 (j - 7)) mod r,
 * w in the device Montgomery form), then 20 words per step-twiddle entry.  *words = its size in 32-bit words (may be
 * NULL); up to max_words of them are copied to out. */
int pm_test_ntt_step4_table(pm_ctx* ctx, uint32_t inverse, uint32_t S, uint32_t* out, size_t max_words, size_t* words);
/* The lazy split table of radix 2^S in form G (G = 1, 2, 3 or 5 data limbs a row; the kernels use 3 and 5) beside it, built on
 * first use: the head, 84 words (word 9 b + j = limb b of w4 2^(29 (j - 8)) mod r), then per entry of the radix-4 steps
 * s >= 2 the rows w 2^(29 (j G + G - 9)) mod r, nine words each, zero words up to a multiple of four (28 words for G = 3).
 * The table of pm_test_ntt_step4_table is not changed by it.  words, max_words and out as there. */
int pm_test_ntt_step4_lazy_table(pm_ctx* ctx, uint32_t inverse, uint32_t S, uint32_t G, uint32_t* out, size_t max_words,
                                 size_t* words);
/* Pure host, no context: thread tid of a radix-4 first or single pass of even radix 2^S (4 <= S <= 10) with 2^LT columns
 * per tile, at its step `step`, in the plane-major exchange of csrc/ntt_kernels4.hip.h (ufast: the pass writes its output
 * u-fast, as a first pass does, which changes the thread order of the last step) -- out[12] = {0 the Stockham butterfly it owns, 1 its column, 2-5 the tile
 * elements it writes X[0..3] to (0xFFFFFFFF at the last step), 6-9 the tile elements it reads its inputs 0..3 from
 * (0xFFFFFFFF at step 0), 10 its step-twiddle digit k', 11 whether the step takes its twiddles from the head's scalar
 * rows (step 1 with a wave-uniform digit)}.  PM_ERR_BAD_ARG for a shape that keeps the Stockham exchange. */
int pm_test_ntt_exchange_map(uint32_t S, uint32_t LT, uint32_t ufast, uint32_t step, uint32_t tid, uint32_t out[12]);
/* Pure host, no context, no device: 1 if pm_fr_ntt* gives this pass launch its fixed-shape kernel, 0 if the generic one.  The launch: a
 * radix-4 pass of radix 2^S over 2^LT columns per tile, role 1 (first) or 3 (last; 0 single and 2 middle have no fixed kernel) of a
 * transform of 2^log_n points of which 2^log_ns are done by the passes before it, intermediate vectors blocked by 2^wide_glog
 * (out[18] of pm_test_ntt_plan), pass_flags the launch's flags (csrc/ntt_kernels.hip.h: 1 PASS_DIRECT_TW, 2 PASS_PRE_COSET,
 * 4 PASS_POST_SCALE, 8 PASS_POST_COSET, 16 PASS_XCD_REMAP, 32 PASS_TW_OUT, 64 PASS_TW_APPLIED, 128 PASS_STEP_PRIO), in_len
 * the elements present in the transform's input, coset whether the transform has PM_NTT_COSET (a transform that is not plain, or
 * pads its input, keeps the generic kernels in all its passes), fixed_shape the option "ntt_fixed_shape" (0, 1 or 2). */
int pm_test_ntt_fixed_match(uint32_t S, uint32_t LT, uint32_t role, uint32_t log_n, uint32_t log_ns, uint32_t wide_glog,
                            uint32_t pass_flags, uint64_t in_len, uint32_t coset, uint32_t fixed_shape);
/* Which kernel each pass of the context's last transform was launched with -- out[4], a pass each: 0 no such pass (sizes below
 * 2^3 have no pass kernels), 1 the generic kernel, 2 its fixed-shape variant. */
int pm_test_ntt_last_variants(pm_ctx* ctx, uint32_t out[4]);
/* Pure host, no context, no device: everything pm_fr_ntt* resolves for a transform before it launches anything -- batch
 * vectors of 2^log_n points with in_len elements present, flags PM_NTT_INVERSE / PM_NTT_COSET.  opts[8] = the options
 * ntt_tile_log, ntt_max_radix, ntt_radix (0 = a fresh context's default, as in pm_test_ntt_plan), then the switches
 * ntt_xcd, ntt_direct_tw, ntt_tw_producer, ntt_step_prio, ntt_fixed_shape (negative = the default: 0 is a value of
 * theirs); num_cus 0 = 256.  out[60] = {0 passes, 1 log2 group size of the blocked intermediate layout, 2 whether the
 * tiny kernel (sizes 2 and 4) runs, 3 its PASS_* flags, 4 whether n^-1 of an inverse transform is folded into the last
 * pass's inter-pass table, 5-7 zero}, then 13 words per pass (up to 4): {log2 radix S, log2 columns per tile LT, role (0
 * single, 1 first, 2 middle, 3 last), kernel family (4 or 8), variant (1 generic, 2 fixed-shape), threads per workgroup,
 * LDS bytes, workgroups per vector, the complete PASS_* flags, log_ns (stages done before the pass), form G of the lazy step
 * table its kernel reads (0: none), the pass whose inter-pass table it reads through pass_tw, the pass whose table it
 * applies to its outputs through pass_tw_out (-1: none)}.  PM_ERR_BAD_ARG also for a pass shape without a kernel. */
int pm_test_ntt_launches(uint32_t log_n, uint32_t batch, uint32_t flags, uint64_t in_len, const long opts[8],
                         uint32_t num_cus, int32_t out[60]);
/* How many device tables the context caches for the NTT: domain and coset tables (a low and a high one each), step tables,
 * lazy step tables and inter-pass tables, both directions. */
int pm_test_ntt_table_count(pm_ctx* ctx, size_t* count);
/* Pure host, no context: the geometry of pm_plonk_sigma_from_wires' sort (csrc/wire_perm.hip) -- passes =
 * max(1, ceil(bits(num_vars - 1) / 8)) 8-bit digit passes, tiles = ceil(4n / 4096) workgroups per pass, scratch_bytes = the
 * transient device memory of the call.  Each out pointer may be NULL.  The errors of pm_plonk_sigma_from_wires for n and
 * num_vars. */
int pm_test_wire_sort_plan(size_t n, size_t num_vars, uint32_t* passes, uint32_t* tiles, size_t* scratch_bytes);
/* Pure host, no context: the digit routine of the fixed-base gadget (csrc/gadgets.hip) compiled for the host.  s: a plain
 * 256-bit integer (not Montgomery), 1 <= rounds <= PM_PLONK_GADGET_MAX_ROUNDS; digits_msb_first[k] = bit_k = e_(rounds-1-k)
 * in {-1, 0, 1}; *too_long (may be NULL) = 1 when some e_j with j >= rounds is non-zero. */
int pm_test_host_naf(const uint64_t s[4], uint32_t rounds, int8_t* digits_msb_first, int* too_long);
/* Pure host, no context: the bucket-fill layout (csrc/msm_sort.hip.h) an MSM of this shape would run with -- out[16] =
 * {window bits, windows, bucket sets, bucket bits, partition bits, local bits, partitions per set, bins, partitions,
 * scalars per scatter tile, tiles, LDS bytes scatter, LDS bytes local sort, finer low partitions, their extra bits, 0} --
 * and, when the three arrays are given (2^bucket-bits / partitions-per-set entries), the partition of every bucket and
 * every partition's first bucket and log2 width.  table_window_bits 0 = bases without a window table. */
int pm_test_msm_geometry(size_t n, long window_bits, uint32_t table_window_bits, uint32_t batch, uint32_t out[16],
                         uint32_t* part_of_bucket, uint32_t* first_bucket, uint32_t* width_bits);
/* Pure host, no context: the scalars of the linearisation polynomial r (csrc/prover_rounds.h, the one copy all provers
 * use) from the 17 evaluations in transcript order (pm_plonk_proof.evaluations; the last, r itself, is not read), the 9
 * further values at z that r(z) needs (q_m, q_o, q_4, z, sigma_4, q_range, q_logic, q_fixed_group_add,
 * q_variable_group_add) and the 10 challenges (pm_plonk_proof.challenges), all Montgomery.  Bit s of
 * selector_present_mask: selector s (the order of pm_plonk_preprocess) is not identically zero; only the four widget
 * selectors' bits matter.  out_count <= 12 terms in the order of the device's linear combination: out_coeffs[i] is the
 * scalar in front of polynomial out_roles[i] = role << 8 | index -- role 2: z, 3: sigma_(index + 1), 4: selector index.
 * out_r_z = r(z) = the sum of coefficient x value at z. */
int pm_test_plonk_linearise(size_t n, const uint64_t (*evaluations)[4], const uint64_t (*extras)[4],
                            const uint64_t (*challenges)[4], uint32_t selector_present_mask, uint64_t (*out_coeffs)[4],
                            uint32_t* out_roles, uint32_t* out_count, uint64_t out_r_z[4]);

#ifdef __cplusplus
}
#endif
#endif /* PLONK_MI355X_H */
