// C++17 host-side mirror of the reference's dependency interface for the hot path, header-only over
// the C ABI of plonk_mi355x.h.  The reference is compiled code (Rust: dusk-plonk 0.8.2 /
// dusk-bls12_381 0.8, ref:Cargo.toml:19-20) and no Rust toolchain exists in the build image, so this
// is the host language the boundary is written in; names, argument meaning and error behaviour
// follow the crates:
//
//   dusk_plonk::fft::EvaluationDomain::{new, fft, ifft, coset_fft, coset_ifft, *_in_place, elements}
//   dusk_bls12_381::multiscalar_mul::msm_variable_base(points, scalars) -> G1Projective
//   dusk_plonk::commitment_scheme::kzg10::CommitKey::{commit, max_degree}   (+ setup, N4)
//   dusk_plonk::fft::Polynomial::{evaluate, ruffini} and coefficient-wise + - *   (device resident)
//
// Memory layouts are the Rust types' own: Fr = BlsScalar([u64; 4]) Montgomery limbs, G1Affine =
// (x, y) of 6 Montgomery limbs each with (0, 0) for the identity, G1Projective = (X, Y, Z).
// Errors: plonk_mi355x::Error carries the pm_status code (InvalidEvalDomainSize = PM_ERR_DOMAIN_TOO_LARGE,
// PolynomialDegreeTooLarge = PM_ERR_LENGTH).  There is no CPU fallback: Context() throws without a
// gfx950 device.  examples/host_demo.cpp exercises everything below.
#ifndef PLONK_MI355X_HPP
#define PLONK_MI355X_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "plonk_mi355x.h"

namespace plonk_mi355x {

using Fr = std::array<uint64_t, 4>;             // dusk_bls12_381::BlsScalar
using G1Affine = std::array<uint64_t, 12>;      // x | y, (0, 0) = identity
using G1Projective = std::array<uint64_t, 18>;  // X | Y | Z, normalised by the library (Z = 1 or (0, 1, 0))

struct Error : std::runtime_error {
  int code;
  uint64_t bad_index = 0;   // PM_ERR_POINT: the lowest failing point ...
  uint32_t bad_reason = 0;  // ... and why (PM_G1_BAD_*)
  Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
  Error(int c, const std::string& what, uint64_t index, uint32_t reason)
      : std::runtime_error(what), code(c), bad_index(index), bad_reason(reason) {}
};

class Context {
 public:
  explicit Context(int device = 0) {
    int rc = pm_init(device, &h_);
    if (rc != PM_OK) throw Error(rc, "pm_init: no usable gfx950 device (there is no CPU fallback)");
  }
  ~Context() { if (h_) pm_shutdown(h_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  pm_ctx* get() const { return h_; }
  void check(int rc) const { if (rc != PM_OK) throw Error(rc, pm_last_error(h_)); }
  void sync() const { check(pm_sync(h_)); }
  // release cached workspaces / twiddle tables (regrown on demand); returns the bytes given back
  size_t trim() const { size_t f = 0; check(pm_trim(h_, &f)); return f; }
  // exchange counters since the last reset (pm_comm_stats): what a multi-GPU deployment pays per proof, countable on one GPU
  struct CommStats { uint64_t alltoall_calls, alltoall_bytes, allgather_calls, transpose_steps; };
  CommStats comm_stats(bool reset = false) const {
    uint64_t v[4];
    check(pm_comm_stats(h_, v, reset ? 1 : 0));
    return CommStats{v[0], v[1], v[2], v[3]};
  }

 private:
  pm_ctx* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
class EvaluationDomain {
 public:
  uint64_t size = 0;
  uint32_t log_size_of_group = 0;
  Fr size_inv{}, group_gen{}, group_gen_inv{};

  // EvaluationDomain::new(num_coeffs): next power of two; Error{PM_ERR_DOMAIN_TOO_LARGE} when
  // log2(size) >= TWO_ADICITY (upstream: Error::InvalidEvalDomainSize)
  EvaluationDomain(Context& ctx, size_t num_coeffs) : ctx_(&ctx) {
    size = 1;
    while (size < num_coeffs) { size <<= 1; ++log_size_of_group; }
    int rc = pm_domain_info(log_size_of_group, group_gen.data(), group_gen_inv.data(), size_inv.data());
    if (rc != PM_OK) throw Error(rc, "InvalidEvalDomainSize: log_size_of_group >= TWO_ADICITY");
  }
  std::vector<Fr> fft(const std::vector<Fr>& coeffs) const { return run(coeffs, 0); }
  std::vector<Fr> ifft(const std::vector<Fr>& evals) const { return run(evals, PM_NTT_INVERSE); }
  std::vector<Fr> coset_fft(const std::vector<Fr>& coeffs) const { return run(coeffs, PM_NTT_COSET); }
  std::vector<Fr> coset_ifft(const std::vector<Fr>& evals) const { return run(evals, PM_NTT_INVERSE | PM_NTT_COSET); }
  void fft_in_place(std::vector<Fr>& a) const { a = run(a, 0); }
  void ifft_in_place(std::vector<Fr>& a) const { a = run(a, PM_NTT_INVERSE); }
  void coset_fft_in_place(std::vector<Fr>& a) const { a = run(a, PM_NTT_COSET); }
  void coset_ifft_in_place(std::vector<Fr>& a) const { a = run(a, PM_NTT_INVERSE | PM_NTT_COSET); }
  // several equal-length polynomials in one call (a prover round): uploads, transforms and downloads overlap
  std::vector<std::vector<Fr>> fft_many(const std::vector<std::vector<Fr>>& polys, uint32_t flags = 0) const {
    if (polys.empty()) return {};
    const size_t len = polys[0].size();
    std::vector<Fr> in(polys.size() * len), out(polys.size() * size);
    for (size_t b = 0; b < polys.size(); ++b) {
      if (polys[b].size() != len) throw Error(PM_ERR_LENGTH, "fft_many: polynomials differ in length");
      std::copy(polys[b].begin(), polys[b].end(), in.begin() + b * len);
    }
    ctx_->check(pm_fr_ntt_batch(ctx_->get(), in.empty() ? nullptr : in[0].data(), len, len, out[0].data(), size,
                                log_size_of_group, (uint32_t)polys.size(), flags));
    std::vector<std::vector<Fr>> res(polys.size());
    for (size_t b = 0; b < polys.size(); ++b) res[b].assign(out.begin() + b * size, out.begin() + (b + 1) * size);
    return res;
  }
  // all domain elements 1, g, g^2, ...
  std::vector<Fr> elements() const {
    std::vector<Fr> x(size > 1 ? 2 : 1, Fr{0, 0, 0, 0});
    x.back() = one();
    return fft(x);
  }
  // evaluate_vanishing_polynomial(tau) = tau^size - 1
  Fr evaluate_vanishing_polynomial(const Fr& tau) const {
    Fr out{};
    int rc = pm_domain_evaluate_vanishing_polynomial(log_size_of_group, tau.data(), out.data());
    if (rc != PM_OK) throw Error(rc, "pm_domain_evaluate_vanishing_polynomial");
    return out;
  }
  // evaluate_all_lagrange_coefficients(tau): [L_0(tau), .., L_(size-1)(tau)]
  std::vector<Fr> evaluate_all_lagrange_coefficients(const Fr& tau) const {
    std::vector<Fr> out(size);
    int rc = pm_domain_evaluate_all_lagrange_coefficients(log_size_of_group, tau.data(), out[0].data());
    if (rc != PM_OK) throw Error(rc, "pm_domain_evaluate_all_lagrange_coefficients");
    return out;
  }
  // compute_vanishing_poly_over_coset(*this, poly_degree): X^poly_degree - 1 on GENERATOR * H, over this domain
  // (upstream asserts size > poly_degree: Error{PM_ERR_BAD_ARG})
  std::vector<Fr> compute_vanishing_poly_over_coset(uint64_t poly_degree) const {
    std::vector<Fr> out(size);
    int rc = pm_domain_vanishing_poly_over_coset(log_size_of_group, poly_degree, out[0].data());
    if (rc != PM_OK) throw Error(rc, "compute_vanishing_poly_over_coset: domain size > poly_degree violated");
    return out;
  }
  static Fr one() { return Fr{0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL, 0x1824b159acc5056fULL}; }

 private:
  std::vector<Fr> run(const std::vector<Fr>& a, uint32_t flags) const {
    if (a.size() > size) throw Error(PM_ERR_LENGTH, "input longer than the domain");
    std::vector<Fr> out(size);
    const Fr zero{0, 0, 0, 0};
    ctx_->check(pm_fr_ntt(ctx_->get(), a.empty() ? zero.data() : a[0].data(), a.size(), out[0].data(),
                          log_size_of_group, flags));
    return out;
  }
  Context* ctx_;
};

// ------------------------------------------------------------------------------------------------
inline G1Affine to_affine(const G1Projective& p, bool* is_identity = nullptr) {
  G1Affine out{};
  int ident = 0;
  int rc = pm_g1_to_affine(p.data(), out.data(), &ident);
  if (rc != PM_OK) throw Error(rc, "pm_g1_to_affine");
  if (is_identity) *is_identity = ident != 0;
  return out;
}

// msm_variable_base(points, scalars): bases uploaded for this one call
inline G1Projective msm_variable_base(Context& ctx, const std::vector<G1Affine>& points, const std::vector<Fr>& scalars) {
  if (points.size() != scalars.size()) throw Error(PM_ERR_LENGTH, "points and scalars differ in length");
  G1Projective out{};
  pm_bases* b = nullptr;
  const G1Affine dummy{};
  ctx.check(pm_g1_bases_upload(ctx.get(), points.empty() ? dummy.data() : points[0].data(), points.size(), &b));
  const Fr zero{0, 0, 0, 0};
  int rc = pm_g1_msm(ctx.get(), b, scalars.size(), scalars.empty() ? zero.data() : scalars[0].data(),
                     PM_SCALAR_MONTGOMERY, out.data());
  pm_g1_bases_free(ctx.get(), b);
  ctx.check(rc);
  return out;
}

class CommitKey {
 public:
  // CommitKey { powers_of_g }: the SRS stays resident in HBM; precompute = also its window table
  CommitKey(Context& ctx, const std::vector<G1Affine>& powers_of_g, bool precompute = false) : ctx_(&ctx) {
    const G1Affine dummy{};
    ctx.check(pm_g1_bases_upload(ctx.get(), powers_of_g.empty() ? dummy.data() : powers_of_g[0].data(),
                                 powers_of_g.size(), &bases_));
    if (precompute) ctx.check(pm_g1_bases_precompute(ctx.get(), bases_, 0));
  }
  ~CommitKey() { if (bases_) pm_g1_bases_free(ctx_->get(), bases_); }
  CommitKey(const CommitKey&) = delete;
  CommitKey& operator=(const CommitKey&) = delete;
  CommitKey(CommitKey&& o) noexcept : ctx_(o.ctx_), bases_(o.bases_) { o.bases_ = nullptr; }
  // CommitKey::from_slice: n x 48 bytes of compressed G1, decoded and checked (encoding, on the curve, and with
  // check_subgroup of order r) on the GPU.  Error{PM_ERR_POINT} carries bad_index / bad_reason
  static CommitKey from_bytes(Context& ctx, const std::vector<uint8_t>& bytes, bool check_subgroup = true,
                              bool precompute = false) {
    if (bytes.size() % 48) throw Error(PM_ERR_LENGTH, "commit key length is not a multiple of 48");
    pm_bases* b = nullptr;
    uint64_t index = 0;
    uint32_t reason = 0;
    const uint8_t dummy = 0;
    const int rc = pm_g1_bases_from_compressed(ctx.get(), bytes.empty() ? &dummy : bytes.data(), bytes.size() / 48,
                                               check_subgroup ? PM_G1_CHECK_SUBGROUP : 0u, &b, &index, &reason);
    if (rc == PM_ERR_POINT) throw Error(rc, pm_last_error(ctx.get()), index, reason);
    ctx.check(rc);
    CommitKey key(ctx, b);
    if (precompute) ctx.check(pm_g1_bases_precompute(ctx.get(), key.bases_, 0));
    return key;
  }
  // CommitKey::to_var_bytes: the powers as n x 48 bytes of compressed G1
  std::vector<uint8_t> to_bytes() const {
    std::vector<uint8_t> out(pm_g1_bases_len(bases_) * 48);
    uint8_t dummy = 0;
    ctx_->check(pm_g1_bases_to_compressed(ctx_->get(), bases_, out.empty() ? &dummy : out.data()));
    return out;
  }
  // for a key loaded raw: every point on the curve (or the identity) and, with subgroup, of order r
  void check(bool subgroup = true) const {
    uint64_t index = 0;
    uint32_t reason = 0;
    const int rc = pm_g1_bases_check(ctx_->get(), bases_, subgroup ? PM_G1_CHECK_SUBGROUP : 0u, &index, &reason);
    if (rc == PM_ERR_POINT) throw Error(rc, pm_last_error(ctx_->get()), index, reason);
    ctx_->check(rc);
  }
  size_t max_degree() const { return pm_g1_bases_len(bases_) - 1; }
  // commit(polynomial): Error{PM_ERR_LENGTH} = PolynomialDegreeTooLarge
  G1Affine commit(const std::vector<Fr>& coeffs) const {
    if (coeffs.size() > pm_g1_bases_len(bases_)) throw Error(PM_ERR_LENGTH, "PolynomialDegreeTooLarge");
    G1Projective p{};
    const Fr zero{0, 0, 0, 0};
    ctx_->check(pm_g1_msm(ctx_->get(), bases_, coeffs.size(), coeffs.empty() ? zero.data() : coeffs[0].data(),
                          PM_SCALAR_MONTGOMERY, p.data()));
    return to_affine(p);
  }
  const pm_bases* bases() const { return bases_; }
  // the Lagrange-form key [L_i(tau)]G of the 2^log_n domain (pm_g1_bases_lagrange): one inverse NTT over the first 2^log_n powers
  // subgroup_points = true: the caller asserts that every power is in the order-r subgroup (a checked key); the twiddle
  // multiplications take the GLV ladder (pm_g1_bases_lagrange_ex).  The same points; undefined outside the subgroup.
  class LagrangeCommitKey lagrange(uint32_t log_n, bool subgroup_points = false) const;
  // The key with powers delta^i P_i: the powers of tau become the powers of tau delta (one contribution to an updatable
  // SRS).  On the device: pm_fr_powers_dev, pm_g1_bases_to_dev, pm_g1_scalar_mul_dev.  Verifying someone else's update
  // needs pairings and is not part of this library.
  CommitKey update(const Fr& delta, bool subgroup_points = false) const {
    const size_t n = pm_g1_bases_len(bases_);
    void *d_xy = nullptr, *d_pow = nullptr;
    ctx_->check(pm_dev_alloc(ctx_->get(), (n ? n : 1) * 96, &d_xy));
    int rc = pm_dev_alloc(ctx_->get(), (n ? n : 1) * 32, &d_pow);
    pm_bases* out = nullptr;
    if (!rc) rc = pm_fr_powers_dev(ctx_->get(), delta.data(), EvaluationDomain::one().data(), n, d_pow, nullptr);
    if (!rc) rc = pm_g1_bases_to_dev(ctx_->get(), bases_, d_xy, nullptr);
    if (!rc) rc = pm_g1_scalar_mul_dev(ctx_->get(), d_xy, d_pow, n, PM_SCALAR_MONTGOMERY,
                                       subgroup_points ? PM_G1_POINTS_IN_SUBGROUP : 0u, d_xy, nullptr);
    if (!rc) rc = pm_g1_bases_from_dev(ctx_->get(), d_xy, n, &out);
    if (d_pow) pm_dev_free(ctx_->get(), d_pow);
    pm_dev_free(ctx_->get(), d_xy);
    ctx_->check(rc);
    return CommitKey(*ctx_, out);
  }

 private:
  CommitKey(Context& ctx, pm_bases* bases) : ctx_(&ctx), bases_(bases) {}
  Context* ctx_;
  pm_bases* bases_ = nullptr;
};

// Commit key in Lagrange form: commit(evals) = the commitment to the polynomial whose values on H are evals (fewer than n
// values are zero padded) -- the same group element CommitKey::commit gives its coefficients.
class LagrangeCommitKey {
 public:
  LagrangeCommitKey(Context& ctx, pm_bases* bases) : ctx_(&ctx), bases_(bases) {}
  ~LagrangeCommitKey() { if (bases_) pm_g1_bases_free(ctx_->get(), bases_); }
  LagrangeCommitKey(const LagrangeCommitKey&) = delete;
  LagrangeCommitKey& operator=(const LagrangeCommitKey&) = delete;
  LagrangeCommitKey(LagrangeCommitKey&& o) noexcept : ctx_(o.ctx_), bases_(o.bases_) { o.bases_ = nullptr; }
  size_t n() const { return pm_g1_bases_len(bases_); }
  G1Affine commit(const std::vector<Fr>& evals) const {
    if (evals.size() > n()) throw Error(PM_ERR_LENGTH, "more evaluations than the domain holds");
    G1Projective p{};
    const Fr zero{0, 0, 0, 0};
    ctx_->check(pm_g1_msm(ctx_->get(), bases_, evals.size(), evals.empty() ? zero.data() : evals[0].data(),
                          PM_SCALAR_MONTGOMERY, p.data()));
    return to_affine(p);
  }
  const pm_bases* bases() const { return bases_; }

 private:
  Context* ctx_;
  pm_bases* bases_ = nullptr;
};

inline LagrangeCommitKey CommitKey::lagrange(uint32_t log_n, bool subgroup_points) const {
  if (log_n >= 32) throw Error(PM_ERR_DOMAIN_TOO_LARGE, "log_n >= 32");
  const size_t n = (size_t)1 << log_n;
  void* d_xy = nullptr;
  ctx_->check(pm_dev_alloc(ctx_->get(), n * 96, &d_xy));
  pm_bases* out = nullptr;
  int rc = subgroup_points ? pm_g1_bases_lagrange_ex(ctx_->get(), bases_, log_n, PM_G1_POINTS_IN_SUBGROUP, d_xy, nullptr)
                           : pm_g1_bases_lagrange(ctx_->get(), bases_, log_n, d_xy, nullptr);
  if (!rc) rc = pm_g1_bases_from_dev(ctx_->get(), d_xy, n, &out);
  pm_dev_free(ctx_->get(), d_xy);
  ctx_->check(rc);
  return LagrangeCommitKey(*ctx_, out);
}

// ------------------------------------------------------------------------------------------------
// dusk_plonk::fft::Polynomial kept in device memory between NTT and MSM calls
class DevicePolynomial {
 public:
  DevicePolynomial(Context& ctx, size_t n) : ctx_(&ctx), n_(n) { ctx.check(pm_dev_alloc(ctx.get(), n * 32, &p_)); }
  DevicePolynomial(Context& ctx, const std::vector<Fr>& coeffs) : DevicePolynomial(ctx, coeffs.size()) {
    if (n_) ctx.check(pm_dev_upload(ctx.get(), p_, coeffs[0].data(), n_ * 32));
  }
  ~DevicePolynomial() { if (p_) pm_dev_free(ctx_->get(), p_); }
  DevicePolynomial(const DevicePolynomial&) = delete;
  DevicePolynomial& operator=(const DevicePolynomial&) = delete;
  DevicePolynomial(DevicePolynomial&& o) noexcept : ctx_(o.ctx_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
  size_t len() const { return n_; }
  void* data() const { return p_; }
  std::vector<Fr> to_host() const {
    std::vector<Fr> out(n_);
    if (n_) ctx_->check(pm_dev_download(ctx_->get(), out[0].data(), p_, n_ * 32));
    return out;
  }
  DevicePolynomial add(const DevicePolynomial& o) const { return op(0, o); }
  DevicePolynomial sub(const DevicePolynomial& o) const { return op(1, o); }
  DevicePolynomial mul(const DevicePolynomial& o) const { return op(2, o); }   // coefficient-wise / scalar (len 1)
  Fr evaluate(const Fr& point) const {
    Fr out{};
    ctx_->check(pm_fr_poly_evaluate_dev(ctx_->get(), p_, n_, point.data(), out.data(), nullptr));
    return out;
  }
  DevicePolynomial ruffini(const Fr& z) const {   // quotient by (X - z), remainder dropped
    DevicePolynomial q(*ctx_, n_ ? n_ - 1 : 0);
    ctx_->check(pm_fr_poly_ruffini_dev(ctx_->get(), p_, n_, z.data(), q.p_, nullptr));
    return q;
  }
  // NTT of the resident coefficients onto a domain of 2^log_n points (zero padded)
  DevicePolynomial ntt(uint32_t log_n, uint32_t flags) const {
    DevicePolynomial out(*ctx_, (size_t)1 << log_n);
    ctx_->check(pm_fr_ntt_dev(ctx_->get(), p_, n_, n_, out.p_, out.n_, log_n, 1, flags, nullptr));
    return out;
  }
  G1Affine commit(const CommitKey& ck) const {
    if (n_ > ck.max_degree() + 1) throw Error(PM_ERR_LENGTH, "PolynomialDegreeTooLarge");
    G1Projective p{};
    ctx_->check(pm_g1_msm_dev(ctx_->get(), ck.bases(), 0, n_, p_, PM_SCALAR_MONTGOMERY, p.data(), nullptr));
    return to_affine(p);
  }

 private:
  DevicePolynomial op(int code, const DevicePolynomial& o) const {
    if (o.n_ != 1 && o.n_ != n_) throw Error(PM_ERR_LENGTH, "operands differ in length");
    DevicePolynomial out(*ctx_, n_);
    ctx_->check(pm_fr_vec_op_dev(ctx_->get(), code, p_, o.p_, o.n_, out.p_, n_, nullptr));
    return out;
  }
  Context* ctx_;
  void* p_ = nullptr;
  size_t n_ = 0;
};

// ------------------------------------------------------------------------------------------------
// dusk_plonk::proof_system::{ProverKey, Prover::preprocess, Prover::prove_with_preprocessed, Proof}: the 11
// selector polynomials of dusk-plonk 0.8 (arithmetic, range, logic, fixed-base, variable-base) and the
// 4-wire permutation; one library call per proof (pm_plonk_prove), everything resident in HBM.
struct Proof {
  std::array<G1Affine, 11> commitments;                  // a b c d z t_1 t_2 t_3 t_4 w_z w_zw
  std::array<Fr, PM_PLONK_EVALS> evaluations;            // transcript order, see plonk_mi355x.h
  std::array<Fr, PM_PLONK_CHALLENGES> challenges;
  std::array<uint8_t, PM_PLONK_PROOF_BYTES> bytes;       // Proof::to_bytes
};
struct PublicInput {
  uint64_t position;   // gate index
  Fr value;
};

class ProverKey;
// pm_plonk_batch: the per-proof workspace of up to max_batch proofs on one key (ProverKey::batch)
class BatchWorkspace {
 public:
  BatchWorkspace(Context& ctx, const pm_prover_key* key, uint32_t max_batch) : ctx_(&ctx), max_batch_(max_batch) {
    ctx.check(pm_plonk_batch_create(ctx.get(), key, max_batch, &ws_));
  }
  ~BatchWorkspace() { if (ws_) pm_plonk_batch_free(ctx_->get(), ws_); }
  BatchWorkspace(const BatchWorkspace&) = delete;
  BatchWorkspace& operator=(const BatchWorkspace&) = delete;
  BatchWorkspace(BatchWorkspace&& o) noexcept : ctx_(o.ctx_), ws_(o.ws_), max_batch_(o.max_batch_) { o.ws_ = nullptr; }
  uint32_t max_batch() const { return max_batch_; }
  size_t device_bytes() const { return pm_plonk_batch_bytes(ws_); }
  // Zero-knowledge batches (pm_plonk_batch_enable_zk; after ProverKey::enable_zk): adds the padded per-proof regions in one
  // allocation (idempotent) and returns the device bytes added.  Plain batches on the workspace are unchanged.
  size_t enable_zk() {
    size_t added = 0;
    ctx_->check(pm_plonk_batch_enable_zk(ctx_->get(), ws_, &added));
    return added;
  }
  pm_plonk_batch* get() const { return ws_; }

 private:
  Context* ctx_;
  pm_plonk_batch* ws_ = nullptr;
  uint32_t max_batch_;
};

class ProverKey {
 public:
  // selectors: q_m q_l q_r q_o q_c q_4 q_arith q_range q_logic q_fixed_group_add q_variable_group_add, n
  // evaluations on H each (an empty vector = identically zero); sigma_index[j n + i] = successor position.
  // The verifier key is committed with `ck` and seeds the transcript every proof starts from.
  ProverKey(Context& ctx, const std::array<std::vector<Fr>, PM_PLONK_SELECTORS>& selectors,
            const std::vector<int64_t>& sigma_index, const CommitKey& ck, const char* transcript_label = nullptr)
      : ctx_(&ctx), n_(selectors[0].size()) {
    const uint64_t* ptrs[PM_PLONK_SELECTORS];
    selector_pointers(selectors, ptrs);
    if (sigma_index.size() != 4 * n_) throw Error(PM_ERR_LENGTH, "sigma_index must have 4n entries");
    ctx.check(pm_plonk_preprocess(ctx.get(), ptrs, sigma_index.data(), n_, &key_));
    commit(ck, transcript_label);
  }
  // The composer's form (pm_plonk_preprocess_wires): wire_vars[j n + i] = the variable at wire j of gate i, an id below
  // num_vars or PM_PLONK_NO_VAR; the copy permutation is built on the device in dusk's order and the key keeps the wire map
  // for witness_from_variables() and enable_check().
  ProverKey(Context& ctx, const std::array<std::vector<Fr>, PM_PLONK_SELECTORS>& selectors,
            const std::vector<uint32_t>& wire_vars, size_t num_vars, const CommitKey& ck, const char* transcript_label = nullptr)
      : ctx_(&ctx), n_(selectors[0].size()) {
    const uint64_t* ptrs[PM_PLONK_SELECTORS];
    selector_pointers(selectors, ptrs);
    if (wire_vars.size() != 4 * n_) throw Error(PM_ERR_LENGTH, "wire_vars must have 4n entries");
    ctx.check(pm_plonk_preprocess_wires(ctx.get(), ptrs, wire_vars.data(), num_vars, n_, &key_));
    commit(ck, transcript_label);
  }
  ~ProverKey() { if (key_) pm_plonk_key_free(ctx_->get(), key_); }
  ProverKey(const ProverKey&) = delete;
  ProverKey& operator=(const ProverKey&) = delete;
  size_t n() const { return n_; }
  const pm_prover_key* get() const { return key_; }
  size_t num_vars() const { return pm_plonk_key_num_vars(key_); }   // 0: the key was built from sigma_index
  const std::array<G1Affine, PM_PLONK_VK_POINTS>& verifier_key() const { return verifier_key_; }
  // batch x var_stride assignments on the device (var_stride >= num_vars()) -> batch x [a | b | c | d] witnesses, proof-major
  // (pm_plonk_witness_from_vars_dev; a key built from wire variables)
  DevicePolynomial witness_from_variables(const DevicePolynomial& variables, size_t var_stride, uint32_t batch = 1) const {
    if (batch == 0 || variables.len() < (size_t)batch * var_stride) throw Error(PM_ERR_LENGTH, "variables must hold batch x var_stride values");
    DevicePolynomial out(*ctx_, (size_t)batch * 4 * n_);
    ctx_->check(pm_plonk_witness_from_vars_dev(ctx_->get(), key_, variables.data(), var_stride, batch, out.data(), nullptr));
    return out;
  }
  // round 1 commits the wires from the witness over lck (checked against ck; nullptr detaches); prove() must then be
  // given the same ck.  The proofs do not change.  lck must outlive the attachment.
  void use_lagrange(const CommitKey& ck, const LagrangeCommitKey* lck) {
    ctx_->check(pm_plonk_key_set_lagrange(ctx_->get(), key_, ck.bases(), lck ? lck->bases() : nullptr));
  }
  // witness: [a | b | c | d] on the device (4n)
  Proof prove(const CommitKey& ck, const DevicePolynomial& witness, const std::vector<PublicInput>& public_inputs = {},
              bool bind_public_inputs = true) const {
    if (witness.len() != 4 * n_) throw Error(PM_ERR_LENGTH, "the witness must hold 4n wire values");
    std::vector<uint64_t> pos, val;
    for (const PublicInput& pi : public_inputs) {
      pos.push_back(pi.position);
      val.insert(val.end(), pi.value.begin(), pi.value.end());
    }
    pm_plonk_proof raw;
    ctx_->check(pm_plonk_prove(ctx_->get(), key_, ck.bases(), witness.data(), pos.data(), val.data(), pos.size(),
                               bind_public_inputs ? 0u : PM_PLONK_UPSTREAM_TRANSCRIPT, &raw));
    return from_raw(raw);
  }
  // Zero-knowledge proofs (pm_plonk_key_enable_zk): builds the key's second 4n coset and the padded workspace once
  // (idempotent); returns the device bytes that state holds.
  size_t enable_zk() {
    size_t added = 0;
    ctx_->check(pm_plonk_key_enable_zk(ctx_->get(), key_, &added));
    return added;
  }
  // A proof that hides the witness (pm_plonk_prove_zk), same format and verifier as prove().  blinders: PM_PLONK_ZK_BLINDERS
  // fresh uniform scalars below r for every proof; ck must hold n + PM_PLONK_ZK_EXTRA_BASES points.
  Proof prove_zk(const CommitKey& ck, const DevicePolynomial& witness, const std::array<Fr, PM_PLONK_ZK_BLINDERS>& blinders,
                 const std::vector<PublicInput>& public_inputs = {}, bool bind_public_inputs = true) const {
    if (witness.len() != 4 * n_) throw Error(PM_ERR_LENGTH, "the witness must hold 4n wire values");
    std::vector<uint64_t> pos, val;
    for (const PublicInput& pi : public_inputs) {
      pos.push_back(pi.position);
      val.insert(val.end(), pi.value.begin(), pi.value.end());
    }
    uint64_t bl[PM_PLONK_ZK_BLINDERS][4];
    for (int i = 0; i < PM_PLONK_ZK_BLINDERS; ++i) std::copy(blinders[i].begin(), blinders[i].end(), bl[i]);
    pm_plonk_proof raw;
    ctx_->check(pm_plonk_prove_zk(ctx_->get(), key_, ck.bases(), witness.data(), pos.data(), val.data(), pos.size(),
                                  bind_public_inputs ? 0u : PM_PLONK_UPSTREAM_TRANSCRIPT, bl, &raw));
    return from_raw(raw);
  }
  // Witness check (pm_plonk_key_enable_check): the selectors on H, the permutation as wire positions (sigma_index: the one
  // the key was built from) and the check's own scratch, once (idempotent); returns the device bytes that state holds.
  size_t enable_check(const std::vector<int64_t>& sigma_index) {
    if (sigma_index.size() != 4 * n_) throw Error(PM_ERR_LENGTH, "sigma_index must have 4n entries");
    size_t added = 0;
    ctx_->check(pm_plonk_key_enable_check(ctx_->get(), key_, sigma_index.data(), &added));
    return added;
  }
  // The same on a key built from wire variables: it rebuilds its own permutation from the wire map.
  size_t enable_check() {
    size_t added = 0;
    ctx_->check(pm_plonk_key_enable_check(ctx_->get(), key_, nullptr, &added));
    return added;
  }
  // Does the witness satisfy the circuit (pm_plonk_check_witness; enable_check() first)?  The report names the lowest failing
  // row and its PM_PLONK_FAIL_* mask; row_masks (optional) receives the mask of every row.
  pm_plonk_witness_report check_witness(const DevicePolynomial& witness, const std::vector<PublicInput>& public_inputs = {},
                                        std::vector<uint8_t>* row_masks = nullptr) const {
    if (witness.len() != 4 * n_) throw Error(PM_ERR_LENGTH, "the witness must hold 4n wire values");
    std::vector<uint64_t> pos, val;
    for (const PublicInput& pi : public_inputs) {
      pos.push_back(pi.position);
      val.insert(val.end(), pi.value.begin(), pi.value.end());
    }
    if (row_masks) row_masks->assign(n_, 0);
    pm_plonk_witness_report report;
    ctx_->check(pm_plonk_check_witness(ctx_->get(), key_, witness.data(), pos.data(), val.data(), pos.size(), &report,
                                       row_masks ? row_masks->data() : nullptr));
    return report;
  }
  // A workspace for prove_batch of up to max_batch (<= PM_PLONK_MAX_BATCH) proofs: about 42 n x 32 bytes per proof
  BatchWorkspace batch(uint32_t max_batch) const { return BatchWorkspace(*ctx_, key_, max_batch); }
  // B proofs in one call: witnesses holds B x [a | b | c | d] (B x 4n, proof-major), public_inputs[b] the inputs of proof b
  // (empty = none for every proof).  Proof b is byte-identical to prove(ck, witness b, public_inputs[b]).
  std::vector<Proof> prove_batch(const CommitKey& ck, BatchWorkspace& ws, const DevicePolynomial& witnesses,
                                 const std::vector<std::vector<PublicInput>>& public_inputs = {},
                                 bool bind_public_inputs = true) const {
    if (witnesses.len() == 0 || witnesses.len() % (4 * n_)) throw Error(PM_ERR_LENGTH, "the witnesses must hold B x 4n wire values");
    const uint32_t B = (uint32_t)(witnesses.len() / (4 * n_));
    if (!public_inputs.empty() && public_inputs.size() != B) throw Error(PM_ERR_LENGTH, "one public-input list per proof");
    std::vector<std::vector<uint64_t>> pos(B), val(B);
    std::vector<const uint64_t*> pp(B, nullptr), vp(B, nullptr);
    std::vector<size_t> cnt(B, 0);
    for (uint32_t b = 0; b < B && !public_inputs.empty(); ++b) {
      for (const PublicInput& pi : public_inputs[b]) {
        pos[b].push_back(pi.position);
        val[b].insert(val[b].end(), pi.value.begin(), pi.value.end());
      }
      cnt[b] = pos[b].size();
      pp[b] = pos[b].data();
      vp[b] = val[b].data();
    }
    std::vector<pm_plonk_proof> raw(B);
    ctx_->check(pm_plonk_prove_batch(ctx_->get(), key_, ws.get(), ck.bases(), B, witnesses.data(), pp.data(), vp.data(),
                                     cnt.data(), bind_public_inputs ? 0u : PM_PLONK_UPSTREAM_TRANSCRIPT, raw.data()));
    std::vector<Proof> out;
    for (const pm_plonk_proof& r : raw) out.push_back(from_raw(r));
    return out;
  }
  // B zero-knowledge proofs in one call (pm_plonk_prove_batch_zk; enable_zk() on the key and on ws first): blinders[b] are
  // proof b's PM_PLONK_ZK_BLINDERS fresh uniform scalars below r -- one independent set per proof, never one for the batch.
  // Proof b is byte-identical to prove_zk(ck, witness b, blinders[b], public_inputs[b]).
  std::vector<Proof> prove_batch_zk(const CommitKey& ck, BatchWorkspace& ws, const DevicePolynomial& witnesses,
                                    const std::vector<std::array<Fr, PM_PLONK_ZK_BLINDERS>>& blinders,
                                    const std::vector<std::vector<PublicInput>>& public_inputs = {},
                                    bool bind_public_inputs = true) const {
    if (witnesses.len() == 0 || witnesses.len() % (4 * n_)) throw Error(PM_ERR_LENGTH, "the witnesses must hold B x 4n wire values");
    const uint32_t B = (uint32_t)(witnesses.len() / (4 * n_));
    if (blinders.size() != B) throw Error(PM_ERR_LENGTH, "one set of blinders per proof");
    if (!public_inputs.empty() && public_inputs.size() != B) throw Error(PM_ERR_LENGTH, "one public-input list per proof");
    std::vector<std::vector<uint64_t>> pos(B), val(B);
    std::vector<const uint64_t*> pp(B, nullptr), vp(B, nullptr);
    std::vector<size_t> cnt(B, 0);
    for (uint32_t b = 0; b < B && !public_inputs.empty(); ++b) {
      for (const PublicInput& pi : public_inputs[b]) {
        pos[b].push_back(pi.position);
        val[b].insert(val[b].end(), pi.value.begin(), pi.value.end());
      }
      cnt[b] = pos[b].size();
      pp[b] = pos[b].data();
      vp[b] = val[b].data();
    }
    std::vector<uint64_t> bl(4 * (size_t)PM_PLONK_ZK_BLINDERS * B);
    for (uint32_t b = 0; b < B; ++b)
      for (int i = 0; i < PM_PLONK_ZK_BLINDERS; ++i)
        std::copy(blinders[b][i].begin(), blinders[b][i].end(), &bl[4 * ((size_t)PM_PLONK_ZK_BLINDERS * b + i)]);
    std::vector<pm_plonk_proof> raw(B);
    ctx_->check(pm_plonk_prove_batch_zk(ctx_->get(), key_, ws.get(), ck.bases(), B, witnesses.data(), pp.data(), vp.data(),
                                        cnt.data(), bind_public_inputs ? 0u : PM_PLONK_UPSTREAM_TRANSCRIPT,
                                        reinterpret_cast<const uint64_t(*)[PM_PLONK_ZK_BLINDERS][4]>(bl.data()), raw.data()));
    std::vector<Proof> out;
    for (const pm_plonk_proof& r : raw) out.push_back(from_raw(r));
    return out;
  }

 private:
  // the selector argument of the two preprocess calls (an empty vector = identically zero)
  void selector_pointers(const std::array<std::vector<Fr>, PM_PLONK_SELECTORS>& selectors,
                         const uint64_t* (&ptrs)[PM_PLONK_SELECTORS]) const {
    for (int s = 0; s < PM_PLONK_SELECTORS; ++s) {
      if (selectors[s].empty()) {
        ptrs[s] = nullptr;
        continue;
      }
      if (selectors[s].size() != n_ || n_ == 0) throw Error(PM_ERR_LENGTH, "selectors differ in length");
      ptrs[s] = selectors[s][0].data();
    }
  }
  // Prover::preprocess's second half: the verifier key, and the transcript every proof starts from
  void commit(const CommitKey& ck, const char* transcript_label) {
    uint64_t vk[PM_PLONK_VK_POINTS][12];
    int rc = pm_plonk_key_commit(ctx_->get(), key_, ck.bases(), transcript_label, vk);
    if (rc) {
      pm_plonk_key_free(ctx_->get(), key_);
      key_ = nullptr;
      ctx_->check(rc);
    }
    for (int i = 0; i < PM_PLONK_VK_POINTS; ++i) std::copy(vk[i], vk[i] + 12, verifier_key_[i].begin());
  }
  Proof from_raw(const pm_plonk_proof& raw) const {
    Proof p;
    for (int i = 0; i < 11; ++i) std::copy(raw.commitments[i], raw.commitments[i] + 12, p.commitments[i].begin());
    for (int i = 0; i < PM_PLONK_EVALS; ++i) std::copy(raw.evaluations[i], raw.evaluations[i] + 4, p.evaluations[i].begin());
    for (int i = 0; i < PM_PLONK_CHALLENGES; ++i) std::copy(raw.challenges[i], raw.challenges[i] + 4, p.challenges[i].begin());
    ctx_->check(pm_plonk_proof_to_bytes(&raw, p.bytes.data()));
    return p;
  }
  Context* ctx_;
  size_t n_;
  pm_prover_key* key_ = nullptr;
  std::array<G1Affine, PM_PLONK_VK_POINTS> verifier_key_;
};

// The same prover with every vector split over `dist.world` ranks by coefficient range (pm_plonk_*_dist, DESIGN.md
// section 7.6): this rank is given its m = n / world rows of every selector column and of the permutation, its slice
// [rank m, (rank + 1) m) of the commit key, and holds 1 / world of the key and workspace.  `dist` carries the two
// collectives (both null: the context's RCCL communicator, pm_comm_init); every rank gets the same proof.
class DistProverKey {
 public:
  DistProverKey(Context& ctx, const pm_dist& dist, const std::array<std::vector<Fr>, PM_PLONK_SELECTORS>& selector_slices,
                const std::vector<int64_t>& sigma_index_slices, size_t n, const CommitKey& ck_slice,
                const char* transcript_label = nullptr)
      : ctx_(&ctx), dist_(dist), n_(n) {
    const size_t m = n / dist.world;
    const uint64_t* ptrs[PM_PLONK_SELECTORS];
    for (int s = 0; s < PM_PLONK_SELECTORS; ++s) {
      if (selector_slices[s].empty()) {
        ptrs[s] = nullptr;
        continue;
      }
      if (selector_slices[s].size() != m) throw Error(PM_ERR_LENGTH, "a selector slice must hold n / world rows");
      ptrs[s] = selector_slices[s][0].data();
    }
    if (sigma_index_slices.size() != 4 * m) throw Error(PM_ERR_LENGTH, "sigma_index_slices must have 4 n / world entries");
    ctx.check(pm_plonk_preprocess_dist(ctx.get(), &dist_, ptrs, sigma_index_slices.data(), n, &key_));
    uint64_t vk[PM_PLONK_VK_POINTS][12];
    int rc = pm_plonk_key_commit_dist(ctx.get(), &dist_, key_, ck_slice.bases(), transcript_label, vk);
    if (rc) {
      pm_plonk_dist_key_free(ctx.get(), key_);
      key_ = nullptr;
      ctx.check(rc);
    }
    for (int i = 0; i < PM_PLONK_VK_POINTS; ++i) std::copy(vk[i], vk[i] + 12, verifier_key_[i].begin());
  }
  ~DistProverKey() { if (key_) pm_plonk_dist_key_free(ctx_->get(), key_); }
  DistProverKey(const DistProverKey&) = delete;
  DistProverKey& operator=(const DistProverKey&) = delete;
  size_t device_bytes() const { return pm_plonk_dist_key_bytes(key_); }
  const std::array<G1Affine, PM_PLONK_VK_POINTS>& verifier_key() const { return verifier_key_; }
  // witness_slices: this rank's [a | b | c | d] rows on the device (4 n / world); public inputs whole, the same on every rank
  Proof prove(const CommitKey& ck_slice, const DevicePolynomial& witness_slices, const std::vector<PublicInput>& public_inputs = {},
              bool bind_public_inputs = true) const {
    if (witness_slices.len() != 4 * (n_ / dist_.world)) throw Error(PM_ERR_LENGTH, "the witness must hold 4 n / world wire values");
    std::vector<uint64_t> pos, val;
    for (const PublicInput& pi : public_inputs) {
      pos.push_back(pi.position);
      val.insert(val.end(), pi.value.begin(), pi.value.end());
    }
    pm_plonk_proof raw;
    ctx_->check(pm_plonk_prove_dist(ctx_->get(), &dist_, key_, ck_slice.bases(), witness_slices.data(), pos.data(), val.data(),
                                    pos.size(), bind_public_inputs ? 0u : PM_PLONK_UPSTREAM_TRANSCRIPT, &raw));
    Proof p;
    for (int i = 0; i < 11; ++i) std::copy(raw.commitments[i], raw.commitments[i] + 12, p.commitments[i].begin());
    for (int i = 0; i < PM_PLONK_EVALS; ++i) std::copy(raw.evaluations[i], raw.evaluations[i] + 4, p.evaluations[i].begin());
    for (int i = 0; i < PM_PLONK_CHALLENGES; ++i) std::copy(raw.challenges[i], raw.challenges[i] + 4, p.challenges[i].begin());
    ctx_->check(pm_plonk_proof_to_bytes(&raw, p.bytes.data()));
    return p;
  }

 private:
  Context* ctx_;
  pm_dist dist_;
  size_t n_;
  pm_dist_key* key_ = nullptr;
  std::array<G1Affine, PM_PLONK_VK_POINTS> verifier_key_;
};

// ------------------------------------------------------------------------------------------------
// Native Poseidon (pm_hades_* / pm_poseidon_*): the constants of one Hades permutation of width 5 on
// the context's GPU and what runs with them -- permutations, the modelled sponge of rate 4, an arity-4 Merkle tree and the
// sibling paths of its leaves.  `form` is PM_HADES_FORM_AUTO, _THREAD or _WAVE; the bytes do not depend on it.
class Hades {
 public:
  // ark: rounds x 5 round keys; mds: 25 entries (one matrix for every round) or rounds x 25
  Hades(Context& ctx, const std::vector<Fr>& ark, const std::vector<Fr>& mds, uint32_t rounds = 67, uint32_t full_rounds = 8)
      : ctx_(&ctx) {
    if (ark.size() != 5 * (size_t)rounds || mds.empty() || mds.size() % 25) throw Error(PM_ERR_LENGTH, "ark: rounds x 5, mds: whole 5 x 5 matrices");
    ctx.check(pm_hades_params_create(ctx.get(), rounds, full_rounds, ark[0].data(), mds[0].data(), (uint32_t)(mds.size() / 25), &p_));
  }
  // the constants of HADES gadget `gadget_index` of the key's gadget table; independent of the key afterwards
  static Hades from_key(Context& ctx, const ProverKey& key, size_t gadget_index) {
    Hades h(ctx);
    ctx.check(pm_hades_params_from_key(ctx.get(), key.get(), gadget_index, &h.p_));
    return h;
  }
  ~Hades() { if (p_) pm_hades_params_free(ctx_->get(), p_); }
  Hades(const Hades&) = delete;
  Hades& operator=(const Hades&) = delete;
  Hades(Hades&& o) noexcept : ctx_(o.ctx_), p_(o.p_) { o.p_ = nullptr; }
  const pm_hades_params* get() const { return p_; }
  uint32_t rounds() const { return info(0); }
  uint32_t full_rounds() const { return info(1); }
  uint32_t n_mds() const { return info(2); }
  // n states of 5 elements, in place; asynchronous on the context's stream
  void permute(DevicePolynomial& states, uint32_t form = PM_HADES_FORM_AUTO) const {
    if (states.len() % 5) throw Error(PM_ERR_LENGTH, "states must hold whole states of 5 elements");
    ctx_->check(pm_hades_permute_dev(ctx_->get(), p_, states.data(), states.len() / 5, form, nullptr));
  }
  std::vector<Fr> permute(const std::vector<Fr>& states, uint32_t form = PM_HADES_FORM_AUTO) const {
    DevicePolynomial d(*ctx_, states);
    permute(d, form);
    return d.to_host();
  }
  // messages.len() / msg_len messages of msg_len elements -> one hash each
  DevicePolynomial hash(const DevicePolynomial& messages, size_t msg_len, const Fr& capacity = Fr{},
                        uint32_t form = PM_HADES_FORM_AUTO) const {
    if (msg_len == 0 || messages.len() % msg_len) throw Error(PM_ERR_LENGTH, "messages must hold whole messages of msg_len >= 1 elements");
    DevicePolynomial out(*ctx_, messages.len() / msg_len);
    ctx_->check(pm_poseidon_hash_dev(ctx_->get(), p_, capacity.data(), messages.data(), msg_len, msg_len, out.len(), out.data(), form,
                                     nullptr));
    return out;
  }
  // 4^height leaves -> levels 1..height one after the other, the root last
  DevicePolynomial merkle(const DevicePolynomial& leaves, uint32_t height, const Fr& capacity = Fr{},
                          uint32_t form = PM_HADES_FORM_AUTO) const {
    if (height < 1 || height > PM_POSEIDON_MERKLE_MAX_HEIGHT || leaves.len() != (size_t)1 << (2 * height))
      throw Error(PM_ERR_LENGTH, "leaves must hold 4^height elements, 1 <= height <= 15");
    DevicePolynomial tree(*ctx_, (leaves.len() - 1) / 3);
    ctx_->check(pm_poseidon_merkle_dev(ctx_->get(), p_, capacity.data(), leaves.data(), height, tree.data(), form, nullptr));
    return tree;
  }
  // out[j][l][c]: child c of the level-(l + 1) ancestor of leaf indices[j]; k x height x 4 elements.  Waits for the stream.
  static std::vector<Fr> merkle_paths(Context& ctx, const DevicePolynomial& leaves, const DevicePolynomial& tree, uint32_t height,
                                      const std::vector<uint64_t>& indices) {
    if (indices.empty()) return {};
    void* d_idx = nullptr;
    ctx.check(pm_dev_alloc(ctx.get(), indices.size() * 8, &d_idx));
    DevicePolynomial out(ctx, indices.size() * height * 4);
    int rc = pm_dev_upload(ctx.get(), d_idx, indices.data(), indices.size() * 8);
    if (!rc) rc = pm_poseidon_merkle_paths_dev(ctx.get(), leaves.data(), tree.data(), height, d_idx, indices.size(), out.data(), nullptr);
    pm_dev_free(ctx.get(), d_idx);
    ctx.check(rc);
    return out.to_host();
  }
  // leaves[indices[j]] = values[j] (indices STRICTLY ASCENDING), then only the ancestors of the changed leaves are hashed
  // again -> the permutations run.  Waits for the stream; a refused call changes nothing.
  uint64_t merkle_update(DevicePolynomial& leaves, DevicePolynomial& tree, uint32_t height, const std::vector<uint64_t>& indices,
                         const std::vector<Fr>& values, const Fr& capacity = Fr{}, uint32_t form = PM_HADES_FORM_AUTO) const {
    if (indices.size() != values.size()) throw Error(PM_ERR_LENGTH, "one value an index");
    if (indices.empty()) return 0;
    const size_t k = indices.size();
    void *d_idx = nullptr, *d_work = nullptr;
    DevicePolynomial d_values(*ctx_, values);
    ctx_->check(pm_dev_alloc(ctx_->get(), k * 8, &d_idx));
    int rc = pm_dev_alloc(ctx_->get(), pm_poseidon_merkle_update_work_bytes(k), &d_work);
    uint64_t hashed = 0;
    if (!rc) rc = pm_dev_upload(ctx_->get(), d_idx, indices.data(), k * 8);
    if (!rc) rc = pm_poseidon_merkle_update_dev(ctx_->get(), p_, capacity.data(), leaves.data(), tree.data(), height, d_idx,
                                                d_values.data(), k, d_work, form, &hashed, nullptr);
    pm_dev_free(ctx_->get(), d_idx);
    if (d_work) pm_dev_free(ctx_->get(), d_work);
    ctx_->check(rc);
    return hashed;
  }
  // paths: k x height x 4 elements as merkle_paths returns them -> a status a path: PM_MERKLE_PATH_OK, _INDEX, _LINK + l
  std::vector<uint32_t> merkle_verify(const std::vector<Fr>& paths, const std::vector<uint64_t>& indices, uint32_t height,
                                      const Fr& root, const Fr& capacity = Fr{}, uint32_t form = PM_HADES_FORM_AUTO) const {
    const size_t k = indices.size();
    if (paths.size() != k * height * 4) throw Error(PM_ERR_LENGTH, "paths must hold k x height x 4 elements");
    std::vector<uint32_t> status(k);
    if (k == 0) return status;
    DevicePolynomial d_paths(*ctx_, paths), d_root(*ctx_, std::vector<Fr>{root});
    void *d_idx = nullptr, *d_status = nullptr;
    ctx_->check(pm_dev_alloc(ctx_->get(), k * 8, &d_idx));
    int rc = pm_dev_alloc(ctx_->get(), k * 4, &d_status);
    if (!rc) rc = pm_dev_upload(ctx_->get(), d_idx, indices.data(), k * 8);
    if (!rc) rc = pm_poseidon_merkle_verify_dev(ctx_->get(), p_, capacity.data(), d_paths.data(), d_idx, k, height, d_root.data(),
                                                d_status, form, nullptr);
    if (!rc) rc = pm_dev_download(ctx_->get(), status.data(), d_status, k * 4);
    pm_dev_free(ctx_->get(), d_idx);
    if (d_status) pm_dev_free(ctx_->get(), d_status);
    ctx_->check(rc);
    return status;
  }
  // no context, no GPU
  static std::array<Fr, 5> permute_host(const std::vector<Fr>& ark, const std::vector<Fr>& mds, std::array<Fr, 5> state,
                                        uint32_t rounds = 67, uint32_t full_rounds = 8) {
    if (ark.size() != 5 * (size_t)rounds || mds.empty() || mds.size() % 25 ||
        pm_hades_permute_host(rounds, full_rounds, ark[0].data(), mds[0].data(), (uint32_t)(mds.size() / 25), state[0].data()))
      throw Error(PM_ERR_BAD_ARG, "pm_hades_permute_host refused its arguments");
    return state;
  }

 private:
  explicit Hades(Context& ctx) : ctx_(&ctx) {}
  uint32_t info(int which) const {
    uint32_t v[3] = {0, 0, 0};
    ctx_->check(pm_hades_params_info(p_, &v[0], &v[1], &v[2]));
    return v[which];
  }
  Context* ctx_;
  pm_hades_params* p_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
// Native JubJub (pm_jubjub_*): one point of the embedded curve on the context's GPU with its window
// table, and what runs with it.  A point is two elements (x, y), the identity (0, 1); scalars are Montgomery elements
// (PM_SCALAR_MONTGOMERY) and multiply as the integers below r they stand for.  Not hardened against side channels.
class JubJubBase {
 public:
  using Point = std::array<Fr, 2>;
  JubJubBase(Context& ctx, const Point& xy) : ctx_(&ctx) { ctx.check(pm_jubjub_base_create(ctx.get(), xy[0].data(), &p_)); }
  // the point FIXED_BASE gadget `gadget_index` of the key's gadget table multiplies; independent of the key afterwards
  static JubJubBase from_key(Context& ctx, const ProverKey& key, size_t gadget_index) {
    JubJubBase b(ctx);
    ctx.check(pm_jubjub_base_from_key(ctx.get(), key.get(), gadget_index, &b.p_));
    return b;
  }
  ~JubJubBase() { if (p_) pm_jubjub_base_free(ctx_->get(), p_); }
  JubJubBase(const JubJubBase&) = delete;
  JubJubBase& operator=(const JubJubBase&) = delete;
  JubJubBase(JubJubBase&& o) noexcept : ctx_(o.ctx_), p_(o.p_) { o.p_ = nullptr; }
  const pm_jubjub_base* get() const { return p_; }
  Point point() const {
    Point xy{};
    ctx_->check(pm_jubjub_base_point(p_, xy[0].data()));
    return xy;
  }
  // n scalars -> n points (2 n elements); asynchronous on the context's stream
  DevicePolynomial mul(const DevicePolynomial& scalars) const {
    DevicePolynomial out(*ctx_, 2 * scalars.len());
    ctx_->check(pm_jubjub_fixed_mul_dev(ctx_->get(), p_, scalars.data(), scalars.len(), PM_SCALAR_MONTGOMERY, out.data(), nullptr));
    return out;
  }
  // out[i] = values[i] * g + blinders[i] * h in one pass
  static DevicePolynomial commit(const JubJubBase& g, const JubJubBase& h, const DevicePolynomial& values, const DevicePolynomial& blinders) {
    if (values.len() != blinders.len()) throw Error(PM_ERR_LENGTH, "one blinder per value");
    DevicePolynomial out(*g.ctx_, 2 * values.len());
    g.ctx_->check(pm_jubjub_commit_dev(g.ctx_->get(), g.p_, h.p_, values.data(), blinders.data(), values.len(), PM_SCALAR_MONTGOMERY,
                                       out.data(), nullptr));
    return out;
  }
  // points[i] <- scalars[i] * points[i], in place; the points are not validated.  Waits for the device.
  static void mul_points(Context& ctx, DevicePolynomial& points, const DevicePolynomial& scalars) {
    if (points.len() != 2 * scalars.len()) throw Error(PM_ERR_LENGTH, "one scalar per point");
    ctx.check(pm_jubjub_mul_dev(ctx.get(), points.data(), scalars.data(), scalars.len(), PM_SCALAR_MONTGOMERY, points.data(), nullptr));
  }
  // the lowest index whose point is off the curve or not canonical; points.len() / 2 when there is none.  Waits for the stream.
  static size_t check(Context& ctx, const DevicePolynomial& points) {
    size_t bad = 0;
    ctx.check(pm_jubjub_check_dev(ctx.get(), points.data(), points.len() / 2, &bad, nullptr));
    return bad;
  }
  // sum scalars[b][i] * points[i] for `batch` scalar vectors at `scalar_stride` elements (0 = n) over the same n points -> batch
  // points (2 batch elements), the bucket method of DESIGN.md section 7.2m; the points are not validated.  Asynchronous.
  static DevicePolynomial msm(Context& ctx, const DevicePolynomial& points, const DevicePolynomial& scalars, uint32_t batch = 1,
                              size_t scalar_stride = 0) {
    const size_t n = points.len() / 2, stride = scalar_stride ? scalar_stride : n;
    if (batch == 0 || stride < n || scalars.len() < (size_t)(batch - 1) * stride + n) throw Error(PM_ERR_LENGTH, "batch vectors of one scalar per point");
    DevicePolynomial out(ctx, 2 * (size_t)batch);
    ctx.check(pm_jubjub_msm_dev(ctx.get(), points.data(), scalars.data(), n, stride, batch, PM_SCALAR_MONTGOMERY, out.data(), nullptr));
    return out;
  }
  // no context, no GPU
  static Point msm_host(const std::vector<Point>& points, const std::vector<Fr>& scalars) {
    Point out{};
    if (points.size() != scalars.size() ||
        pm_jubjub_msm_host(points.empty() ? nullptr : points[0][0].data(), scalars.empty() ? nullptr : scalars[0].data(), points.size(),
                           PM_SCALAR_MONTGOMERY, out[0].data()))
      throw Error(PM_ERR_BAD_ARG, "pm_jubjub_msm_host refused its arguments");
    return out;
  }
  static Point mul_host(const Point& xy, const Fr& scalar) {
    Point out{};
    if (pm_jubjub_mul_host(xy[0].data(), scalar.data(), PM_SCALAR_MONTGOMERY, out[0].data())) throw Error(PM_ERR_BAD_ARG, "pm_jubjub_mul_host refused its arguments");
    return out;
  }
  static Point add_host(const Point& p, const Point& q) {
    Point out{};
    if (pm_jubjub_add_host(p[0].data(), q[0].data(), out[0].data())) throw Error(PM_ERR_BAD_ARG, "pm_jubjub_add_host refused its arguments");
    return out;
  }

 private:
  explicit JubJubBase(Context& ctx) : ctx_(&ctx) {}
  Context* ctx_;
  pm_jubjub_base* p_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
// Native Schnorr signatures on JubJub (pm_schnorr_*): u G + c PK = R with c = H(R.x, R.y, m) below 2^250.
// g must have order exactly JUBJUB_ORDER.  A signature is three elements (u, R.x, R.y); secret keys, nonces and u are Montgomery
// elements (PM_SCALAR_MONTGOMERY).  The nonces are the caller's: the library has no random number generator.  Signing is not
// hardened against side channels.  The base and the constants must outlive this object.
class Schnorr {
 public:
  Schnorr(Context& ctx, const JubJubBase& g, const Hades& hades, const Fr& capacity = Fr{}) : ctx_(&ctx), g_(&g), h_(&hades), cap_(capacity) {}
  // n secret keys, nonces and messages -> 3 n elements; asynchronous on the context's stream
  DevicePolynomial sign(const DevicePolynomial& secret_keys, const DevicePolynomial& nonces, const DevicePolynomial& messages) const {
    if (secret_keys.len() != nonces.len() || secret_keys.len() != messages.len()) throw Error(PM_ERR_LENGTH, "one nonce and one message per key");
    DevicePolynomial out(*ctx_, 3 * secret_keys.len());
    ctx_->check(pm_schnorr_sign_dev(ctx_->get(), g_->get(), h_->get(), cap_.data(), secret_keys.data(), nonces.data(), messages.data(),
                                    secret_keys.len(), PM_SCALAR_MONTGOMERY, out.data(), nullptr));
    return out;
  }
  // the lowest index whose signature is not valid; messages.len() when every one is.  Waits for the device.
  size_t verify(const DevicePolynomial& public_keys, const DevicePolynomial& messages, const DevicePolynomial& signatures) const {
    if (public_keys.len() != 2 * messages.len() || signatures.len() != 3 * messages.len()) throw Error(PM_ERR_LENGTH, "one key and one signature per message");
    size_t bad = 0;
    ctx_->check(pm_schnorr_verify_dev(ctx_->get(), g_->get(), h_->get(), cap_.data(), public_keys.data(), messages.data(), signatures.data(),
                                      messages.len(), PM_SCALAR_MONTGOMERY, nullptr, &bad, nullptr));
    return bad;
  }
  // ONE cofactored equation for all signatures (pm_schnorr_verify_batch_dev) under the caller's weights: n x 16 bytes on the
  // device, 0 < z_i < 2^128, fresh and unpredictable.  Weaker than verify (the header); true = accepted.  On false, *reason
  // and *first_bad (either may be null) say why: a structural reason and its index, or PM_SCHNORR_EQUATION and n.  Waits.
  bool verify_batch(const DevicePolynomial& public_keys, const DevicePolynomial& messages, const DevicePolynomial& signatures,
                    const void* d_weights, uint32_t* reason = nullptr, size_t* first_bad = nullptr) const {
    if (public_keys.len() != 2 * messages.len() || signatures.len() != 3 * messages.len()) throw Error(PM_ERR_LENGTH, "one key and one signature per message");
    uint32_t r = 0;
    size_t bad = 0;
    ctx_->check(pm_schnorr_verify_batch_dev(ctx_->get(), g_->get(), h_->get(), cap_.data(), public_keys.data(), messages.data(),
                                            signatures.data(), d_weights, messages.len(), PM_SCALAR_MONTGOMERY, nullptr, &r, &bad, nullptr));
    if (reason) *reason = r;
    if (first_bad) *first_bad = bad;
    return r == PM_SCHNORR_OK;
  }

 private:
  Context* ctx_;
  const JubJubBase* g_;
  const Hades* h_;
  Fr cap_;
};

}  // namespace plonk_mi355x
#endif  // PLONK_MI355X_HPP
