// One Fr transform split over ranks (pm_fr_ntt_fourstep*_dev): the pack / unpack kernels of its transposes and the driver
// that strings them, the all-to-all exchanges and the library's own batched sub-transforms together.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ntt_internal.h"
#include "ntt_kernels.hip.h"

// ------------------------------------------------------------------ N5: one transform split over ranks
// SURVEY.md section 8e row 3 / 8f N5.  The vector of a 2^log_n-point transform is block-distributed in natural
// order over `world` ranks (one process and one pm_ctx per GPU): rank r holds x[r N/W, (r+1) N/W) and receives the
// same block of the result.  N = N1 N2 as an N1 x N2 row-major matrix (N1 = 2^(log_n / 2)):
//     transpose (all-to-all) -> N2/W batched transforms of size N1 -> twiddles w_N^(j k1)
//     -> transpose -> N1/W batched transforms of size N2 -> transpose (natural order)
// A transpose is: pack this rank's [R_loc][C] slice into per-peer blocks [peer][C/W][R_loc] (a 32 x 32 tile
// transpose through LDS; the twiddle / coset factors are folded into this pass), one all-to-all of N/W^2-element
// blocks (the context's RCCL communicator: grouped ncclSend / ncclRecv, one direct xGMI transfer per peer -- or a
// caller-supplied callback), and an unpack that interleaves what the peers sent into [C/W][R].  The sub-transforms
// are the library's own batched passes.  Results are identical to the single-GPU plan bit for bit.
namespace pm {

struct FsMul {            // factor applied to element (row a, column b) of the slice while it is packed / unpacked
  u32 mode;               // 0 none, 1 table^((row0 + a) * b)  (twiddle), 2 table^((row0 + a) * C + b)  (coset by index)
  const u32x4* hi;
  const u32x4* lo;
  u32 lh;
  u32 row0;
};
PM_DEV void fs_apply(u32x4& v0, u32x4& v1, const FsMul& m, u32 a, u32 b, u32 C) {
  if (m.mode == 0) return;
  const u32 e = m.mode == 1 ? (m.row0 + a) * b : (m.row0 + a) * C + b;
  u32x4 raw[2] = {v0, v1};
  Fr x = fe_load<FrP>(raw);
  x = fe_mul<FrP>(x, two_level(m.hi, m.lo, e, m.lh));
  fe_store<FrP>(raw, x);
  v0 = raw[0];
  v1 = raw[1];
}
// A transpose step works on `batch` vectors at once: the per-peer block of the all-to-all holds the batch's blocks one
// after the other, so ONE exchange carries all of them (message size x batch, call count / batch).
// send[((s * batch + v) * Cs + bl) * R_loc + a] = f(src_v[a * C + s * Cw + bl]),  s = b / Cw, bl = b % Cw;  Cs = Cw, or Cw + 1
// with `halo`: the block for rank s then ends with one more column, (s + 1) Cw mod C -- the first column of the NEXT
// rank's range (the last rank gets column 0) -- which the unpack turns into one extra row.
__global__ void __launch_bounds__(256) fs_pack_kernel(const u32x4* src, size_t src_stride, u32 batch, u32 R_loc, u32 C, u32 Cw,
                                                      u32 halo, u32x4* send, const FsMul m) {
  __shared__ u32x4 t0[32][33], t1[32][33];
  const u32 v = blockIdx.z;
  src += 2 * (size_t)v * src_stride;
  const u32 a0 = blockIdx.y * 32, b0 = blockIdx.x * 32;
  const u32 tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;   // 32 x 8
  for (u32 r = ty; r < 32; r += 8) {
    const u32 a = a0 + r, b = b0 + tx;
    if (a < R_loc && b < C) {
      u32x4 v0 = src[2 * ((size_t)a * C + b)], v1 = src[2 * ((size_t)a * C + b) + 1];
      fs_apply(v0, v1, m, a, b, C);
      t0[r][tx] = v0;
      t1[r][tx] = v1;
    }
  }
  __syncthreads();
  const u32 Cs = Cw + halo, W = C / Cw;
  for (u32 r = ty; r < 32; r += 8) {
    const u32 b = b0 + r, a = a0 + tx;
    if (a < R_loc && b < C) {
      const u32 s = b / Cw, bl = b % Cw;
      const size_t o = (((size_t)s * batch + v) * Cs + bl) * R_loc + a;
      send[2 * o] = t0[tx][r];
      send[2 * o + 1] = t1[tx][r];
      if (halo && bl == 0) {   // also the extra column of the rank before s
        const u32 sp = (s + W - 1) % W;
        const size_t oh = (((size_t)sp * batch + v) * Cs + Cw) * R_loc + a;
        send[2 * oh] = t0[tx][r];
        send[2 * oh + 1] = t1[tx][r];
      }
    }
  }
}
// dst_v[bl * R + p * R_loc + a] = g(recv[((p * batch + v) * Cs + bl) * R_loc + a]),  R = W R_loc; g's index: row bl, column
// p R_loc + a.  With halo the extra row bl == Cw goes to halo_v[p * R_loc + a] instead.
__global__ void __launch_bounds__(256) fs_unpack_kernel(const u32x4* recv, u32 batch, u32 R_loc, u32 W, u32 Cw, u32 halo,
                                                        u32x4* dst, size_t dst_stride, u32x4* halo_dst, const FsMul m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 v = blockIdx.y;
  const u32 R = R_loc * W, Cs = Cw + halo;
  if (t >= (size_t)Cs * R) return;
  const u32 bl = (u32)(t / R), rr = (u32)(t % R), p = rr / R_loc, a = rr % R_loc;
  const size_t i = (((size_t)p * batch + v) * Cs + bl) * R_loc + a;
  u32x4 v0 = recv[2 * i], v1 = recv[2 * i + 1];
  fs_apply(v0, v1, m, bl, rr, R);
  u32x4* o = bl < Cw ? dst + 2 * ((size_t)v * dst_stride + t) : halo_dst + 2 * ((size_t)v * R + rr);
  o[0] = v0;
  o[1] = v1;
}

}  // namespace pm

using namespace pm;

extern "C" int pm_fr_ntt_fourstep_batch_dev(pm_ctx* ctx, void* d_inout, uint32_t batch, void* d_halo, void* d_stage,
                                            uint32_t log_n, uint32_t world, uint32_t rank, uint32_t flags,
                                            pm_alltoall_fn exchange, void* user) {
  if (!ctx || !d_inout || !d_stage || batch == 0) return PM_ERR_BAD_ARG;
  if (world == 0 || (world & (world - 1)) || rank >= world) return PM_ERR_BAD_ARG;
  if (flags & ~(PM_NTT_INVERSE | PM_NTT_COSET | PM_NTT_TRANSPOSED)) return PM_ERR_BAD_ARG;
  if (log_n < 2 || log_n > 26) return PM_ERR_DOMAIN_TOO_LARGE;   // 32-bit exponents of the two-level tables
  const uint32_t l1 = log_n / 2, l2 = log_n - l1;
  const uint32_t n1 = 1u << l1, n2 = 1u << l2;
  if (n1 % world || n2 % world) return PM_ERR_BAD_ARG;            // the ranks must divide both factors
  const bool inverse = flags & PM_NTT_INVERSE, coset = flags & PM_NTT_COSET;
  const bool want_halo = d_halo != nullptr;
  if (want_halo && (inverse || !(flags & PM_NTT_TRANSPOSED))) return PM_ERR_BAD_ARG;   // a row of the block-transposed result
  const size_t blk = ((size_t)1 << log_n) / world;                // elements per rank and vector
  if (batch > 65535u) return PM_ERR_BAD_ARG;
  u32x4* x = (u32x4*)d_inout;
  u32x4* send = (u32x4*)d_stage;
  // stage: [send | recv], each batch x (blk, or blk + n2 with a halo row) elements; one rank needs no recv half
  const size_t stage_half = (size_t)batch * (blk + (want_halo ? n2 : 0));
  u32x4* recv = world == 1 ? send : send + 2 * stage_half;
  hipStream_t st;
  NttDomainTables* dt = nullptr;
  // the transform holds the NTT resource group from here to its last launch, with the context unlocked in between (the
  // exchange callback): the scope's closing event is recorded, under the lock, when the function returns
  struct HeldOrder {
    pm_ctx* ctx;
    OrderScope* s;
    ~HeldOrder() {
      if (!s) return;
      std::lock_guard<std::mutex> lk(ctx->mu);
      delete s;
      --ctx->calls_holding_tables;
    }
  } held{ctx, nullptr};
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    PM_HIP(ctx, hipSetDevice(ctx->device));
    st = ctx->stream;
    if (world > 1 && !exchange && (!ctx->comm || ctx->comm_world != (int)world || ctx->comm_rank != (int)rank))
      return set_err(ctx, PM_ERR_EXCHANGE, "no exchange callback and no matching communicator (pm_comm_init)");
    held.s = new OrderScope(ctx, ctx->ord_ntt, st);
    ++ctx->calls_holding_tables;   // dt and the tables behind it stay in use across the unlocked exchange steps: no pm_trim
    int rc = held.s->rc;
    if (!rc) rc = get_domain_tables(ctx, inverse ? 1 : 0, log_n, coset, &dt, st);
    if (rc) return rc;
  }
  const FsMul none{0, nullptr, nullptr, 0, 0};
  // one transpose of every vector of the batch: slice [R_loc][C] of a row-distributed [R][C] matrix -> slice [C / W][R]
  // of its transpose (+ one halo row).  The result is in *where: x -- or, with one rank and no factor on the way in, the
  // stage buffer itself (the unpack would be a plain copy: the next sub-transform reads it from there; `keep_in_x`
  // forces the copy)
  auto transpose = [&](const u32x4* from, u32 R_loc, u32 C, const FsMul& on_pack, const FsMul& on_unpack, bool keep_in_x,
                       bool halo, const u32x4** where) -> int {
    const u32 Cw = C / world, Cs = Cw + (halo ? 1u : 0u);
    const size_t peer_bytes = (size_t)batch * Cs * R_loc * 32;
    {
      std::lock_guard<std::mutex> lk(ctx->mu);
      ProfScope prof(ctx, st, "ntt_fourstep_transpose");
      hipLaunchKernelGGL(fs_pack_kernel, dim3((C + 31) / 32, (R_loc + 31) / 32, batch), dim3(256), 0, st, from, blk, batch, R_loc,
                         C, Cw, halo ? 1u : 0u, send, on_pack);
      PM_HIP(ctx, hipGetLastError());
      ++ctx->stat_transpose_steps;
      if (world > 1) {
        ++ctx->stat_alltoall_calls;
        ctx->stat_alltoall_bytes += peer_bytes * (world - 1);
      }
      if (world > 1 && !exchange) {
        int rc = comm_alltoall(ctx, send, recv, peer_bytes, st);
        if (rc) return rc;
      }
    }
    if (world == 1 && on_unpack.mode == 0 && !keep_in_x && !halo) {
      *where = send;
      return PM_OK;
    }
    if (world > 1 && exchange) {   // the callback sees finished data and returns when the peers' blocks are in place
      {
        std::lock_guard<std::mutex> lk(ctx->mu);
        PM_HIP(ctx, hipStreamSynchronize(st));
      }
      if (exchange(user, send, recv, peer_bytes) != 0) return set_err(ctx, PM_ERR_EXCHANGE, "the all-to-all callback failed");
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ProfScope prof(ctx, st, "ntt_fourstep_transpose");
    const size_t total = (size_t)Cs * R_loc * world;
    hipLaunchKernelGGL(fs_unpack_kernel, dim3((unsigned)((total + 255) / 256), batch), dim3(256), 0, st, (const u32x4*)recv, batch,
                       R_loc, world, Cw, halo ? 1u : 0u, x, blk, (u32x4*)d_halo, on_unpack);
    PM_HIP(ctx, hipGetLastError());
    *where = x;
    return PM_OK;
  };
  const uint32_t sub = inverse ? PM_NTT_INVERSE : 0;
  // PM_NTT_TRANSPOSED: a forward transform leaves its result as the [N1 / W][N2] matrix of step 4 -- X[k2 N1 + k1] at
  // position k1 N2 + k2, rank r holding rows k1 in [r N1 / W, (r + 1) N1 / W) -- and skips the third all-to-all; an
  // inverse transform TAKES that layout: with the two factors swapped it is exactly the state after step 1.  What sits
  // between the two in a prover (the pointwise quotient) does not care about the order.
  const bool transposed = flags & PM_NTT_TRANSPOSED;
  const uint32_t la = transposed && inverse ? l2 : l1, lb = log_n - la;   // rows x columns of the input matrix
  const uint32_t na = 1u << la, nb = 1u << lb;
  const u32x4* cur = x;
  int rc = PM_OK;
  if (!(transposed && inverse)) {
    // 1: [A/W][B] -> [B/W][A]  (coset_fft: x[n] *= g^n on the way out)
    FsMul pre = none;
    if (coset && !inverse) pre = FsMul{2, (const u32x4*)dt->cs_hi, (const u32x4*)dt->cs_lo, dt->lh, rank * (na / world)};
    rc = transpose(x, na / world, nb, pre, none, false, false, &cur);
    if (rc) return rc;
  }
  // `count` contiguous transforms of 2^lg points, in -> out (the batched passes put the batch on gridDim.y: at most 65535 per launch)
  auto sub_ntts = [&](const void* in, void* out, uint32_t lg, size_t count) -> int {
    const size_t len = (size_t)1 << lg;
    for (size_t done = 0; done < count;) {
      const uint32_t now = (uint32_t)std::min<size_t>(count - done, 32768);
      int r = pm_fr_ntt_dev(ctx, (const char*)in + done * len * 32, len, len, (char*)out + done * len * 32, len, lg, now, sub, nullptr);
      if (r) return r;
      done += now;
    }
    return PM_OK;
  };
  // 2: B/W transforms of size A over the columns, every vector of the batch (the blocks are contiguous)
  rc = sub_ntts(cur, x, la, (size_t)batch * (nb / world));
  if (rc) return rc;
  // 3: [B/W][A] -> [A/W][B], element (j, k1) times w^(j k1) on the way out; with a halo one more row: the next rank's first
  const FsMul tw{1, (const u32x4*)dt->tw_hi, (const u32x4*)dt->tw_lo, dt->lh, rank * (nb / world)};
  rc = transpose(x, nb / world, na, tw, none, false, want_halo, &cur);
  if (rc) return rc;
  // 4: A/W transforms of size B over the rows (and over the halo rows: one per vector, contiguous in d_halo)
  rc = sub_ntts(cur, x, lb, (size_t)batch * (na / world));
  if (rc) return rc;
  if (want_halo) {
    rc = sub_ntts(d_halo, d_halo, lb, batch);
    if (rc) return rc;
  }
  if (transposed && !inverse) return PM_OK;
  // 5: [A/W][B] (k1, k2) -> [B/W][A] (k2, k1) = natural order  (coset_ifft: X[k] *= g^-k on the way in)
  FsMul post = none;
  if (coset && inverse) post = FsMul{2, (const u32x4*)dt->cs_hi, (const u32x4*)dt->cs_lo, dt->lh, rank * (nb / world)};
  return transpose(x, na / world, nb, none, post, true, false, &cur);
}

extern "C" int pm_fr_ntt_fourstep_dev(pm_ctx* ctx, void* d_inout, void* d_stage, uint32_t log_n, uint32_t world,
                                      uint32_t rank, uint32_t flags, pm_alltoall_fn exchange, void* user) {
  return pm_fr_ntt_fourstep_batch_dev(ctx, d_inout, 1, nullptr, d_stage, log_n, world, rank, flags, exchange, user);
}
