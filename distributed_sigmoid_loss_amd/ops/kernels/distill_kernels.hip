// Sigmoid distillation loss for gfx950 (MI355X): the sigmoid loss against soft
// targets that come from a teacher dual encoder's own pair grid, mixed with
// the hard positional label.  Two (b, n) grids of dot products — the
// teacher's and the student's — are evaluated tile by tile in one kernel, and
// neither is ever written to memory.
//
//   s_ij = <zimg_i, ztxt_j>        z_ij = t·s_ij + bias,        t   = exp(t')
//   u_ij = <timg_i, ttxt_j>        p_ij = σ(t_T·u_ij + bias_T), t_T = exp(t'_T)
//   q_ij = alpha·p_ij + (1 − alpha)·[j == i + diag]
//   term = softplus(z) − q·z       g = σ(z) − q
//
// One tile body template <WRITE_G>, two kernels.  Both leave three fp32
// partials per 128×128 tile — Σ term, Σ g·s, Σ g — in a (tiles, 3) workspace;
// <true> also stages the bf16 g tile in LDS and writes it as coalesced
// 16-byte row segments into a (b, n) view of row stride ldg.  The partials of
// the two are bit-identical: they come from the fp32 g, the arithmetic is the
// same sequence of explicit fmas, and every reduction has a fixed order (xor
// shuffles, then the four waves in wave order).  No atomics, no counters.
//
// Two K loops, one LDS.  pair_tile.h's main loop runs twice in the same
// 64 KiB of operand slabs (it ends on a barrier, so the second run may
// overwrite what the first one staged): first over the teacher pair
// (timg, ttxt, d_T), then over the student pair (zimg, ztxt, d).  d and d_T
// are independent, each with its own zero-filled K tail.  Between the two the
// teacher's 64 accumulators are turned in place into the targets q, which
// stay there as fp32 across the student loop: the slabs take all of the LDS,
// and a packed bf16 q would put 2⁻⁹ into a g that is the difference of two
// probabilities.  A lane thus holds 128 accumulators, 64 of them live in the
// MFMA at any time; with the staging registers that is still two workgroups
// per CU (__launch_bounds__(256, 2): 256 VGPRs + AGPRs per lane), which hide
// each other's conversion and epilogue.
//
// MXFP8 teacher (sigmoid_distill_kernel<WRITE_G, mx_e4m3>).  The teacher gets
// no gradient and enters no gradient GEMM, so it may be stored as e4m3 bytes
// with one e8m0 scale per 32 k (ops.quantize_mx).  Its K loop is then
// pair_tile.h's MX main loop — half the K-steps and barriers, half the bytes
// per k, v_mfma_scale_f32_16x16x128_f8f6f4 applying the scales, so u is the
// true dot of the dequantised values and t'_T, bias_T are unchanged — and
// everything from the target conversion on is the same code.  During that
// loop only the 64 teacher accumulators are live, so its resident text
// fragments and scales have room.  LDS is MX_LDS_BYTES (66 KiB; two
// workgroups are 132 of 160 KiB): the scale area lies above everything the
// student loop and the epilogue staging use, and the MX loop ends on a
// barrier, so the student's first stage overwrites the teacher's last slabs
// with no barrier added.
//
// The hard label is folded into q at the conversion — q = fma(alpha, p, hard)
// with hard = 1 − alpha on the lane's positive column and 0 elsewhere — so
// the epilogue knows nothing of positions, and alpha = 0 gives q = [j == i +
// diag] exactly: the positional sigmoid loss.
//
// Epilogue (column-major over the fragments, as in idlabel_kernels.hip).
// With e = exp(−|z|):
//   term = log(1 + e) + (z > 0 ? (1 − q)·z : −q·z)
// is softplus(z) − q·z as a sum of two non-negative parts (0 ≤ q ≤ 1), so a
// confident pair with q near σ(z) loses nothing to cancellation, and
//   g = (z ≥ 0 ? 1 : e) / (1 + e) − q.
// A row ≥ b or a column ≥ n contributes nothing: a zero-filled padding
// element has z = bias, not 0, and would add softplus(bias) − q·bias.
//
// exp / log are the bare v_exp_f32 / v_log_f32 (base 2) with the ln 2 factors
// folded in; 1 / (1 + e) is v_rcp_f32 (1 ulp, 2⁻¹⁶ of a bf16 ulp).

#include "pair_tile.h"

#include <type_traits>

namespace {

// 4 waves × 3 partials above the g staging.
constexpr int RED_OFF = G_STAGE_BYTES;
static_assert(RED_OFF + 64 <= 2 * BUF_BYTES, "epilogue staging exceeds LDS");

// σ(x) without a branch on the sign of x and without an overflow.
__device__ __forceinline__ float sigmoid_f32(float x) {
  const float e = __builtin_amdgcn_exp2f(-__builtin_fabsf(x) * LOG2E);
  return (x >= 0.f ? 1.f : e) * __builtin_amdgcn_rcpf(1.f + e);
}

// TOP is the teacher's operand element: __bf16, or mx_e4m3 with the block
// scales in timg_e8 / ttxt_e8, rows lde bytes apart (unused for __bf16).
template <bool WRITE_G, typename TOP = __bf16>
__launch_bounds__(NTHREADS, 2) __global__ void sigmoid_distill_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const float* __restrict__ bias,
    const TOP* __restrict__ timg, const TOP* __restrict__ ttxt,
    const float* __restrict__ tprime_t, const float* __restrict__ bias_t,
    __bf16* __restrict__ g, float* __restrict__ ws, int b, int n, int d,
    int d_t, long long ldg, int diag, float alpha, int tiles_m, int tiles_n,
    const unsigned char* __restrict__ timg_e8,
    const unsigned char* __restrict__ ttxt_e8, int lde) {
  constexpr bool MX_T = std::is_same<TOP, mx_e4m3>::value;
  __shared__ __attribute__((aligned(16))) unsigned char
      lds[MX_T ? MX_LDS_BYTES : 2 * BUF_BYTES];
  const TilePos tp = tile_of_block(tiles_m, tiles_n);
  const int m0 = tp.tm * BM, n0 = tp.tn * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;

  // Teacher: dots, then the targets in place.
  f32x4 q[4][4];
  if constexpr (MX_T)
    pair_tile_dots_mx<true>((const unsigned char*)timg, timg_e8,
                            (const unsigned char*)ttxt, ttxt_e8, b, n, d_t,
                            lde, m0, n0, lds, q);
  else
    pair_tile_dots<true>(timg, ttxt, b, n, d_t, m0, n0, lds, q);
  {
    const float tt = expf(tprime_t[0]);
    const float bt = bias_t[0];
    const float hard_w = 1.f - alpha;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pc = positive_col(m0 + wm * 64 + i * 16 + fr, diag, n);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col0 = n0 + wn * 64 + j * 16 + fq * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = sigmoid_f32(__builtin_fmaf(q[i][j][r], tt, bt));
          q[i][j][r] =
              __builtin_fmaf(alpha, p, col0 + r == pc ? hard_w : 0.f);
        }
      }
    }
  }

  // Student: the same LDS, a second accumulator set.
  f32x4 acc[4][4];
  pair_tile_dots<true>(zimg, ztxt, b, n, d, m0, n0, lds, acc);

  const float t = expf(tprime[0]);
  const float bs = bias[0];
  bool row_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) row_ok[i] = m0 + wm * 64 + i * 16 + fr < b;

  float s_loss = 0.f, s_gs = 0.f, s_g = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int lcol0 = wn * 64 + j * 16 + fq * 4;
    const int col0 = n0 + lcol0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x4 out;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[i][j][r];
        const float qv = q[i][j][r];
        const float z = __builtin_fmaf(s, t, bs);
        const float e = __builtin_amdgcn_exp2f(-__builtin_fabsf(z) * LOG2E);
        const float den = 1.f + e;
        const float lg = LN2 * __builtin_amdgcn_logf(den);
        // (1 − q)·z for z > 0, −q·z otherwise: both ≥ 0.
        const float w = z > 0.f ? 1.f - qv : -qv;
        float term = __builtin_fmaf(w, z, lg);
        float gv = (z >= 0.f ? 1.f : e) * __builtin_amdgcn_rcpf(den) - qv;
        if (!row_ok[i] || col0 + r >= n) {
          term = 0.f;
          gv = 0.f;
        }
        s_loss += term;
        s_gs = __builtin_fmaf(gv, s, s_gs);
        s_g += gv;
        if (WRITE_G) out[r] = (__bf16)gv;
      }
      if (WRITE_G)
        *reinterpret_cast<bf16x4*>(lds + (wm * 64 + i * 16 + fr) * G_PITCH
                                   + 2 * lcol0) = out;
    }
  }

  // The tile's three sums: lanes by xor shuffles, then the four waves in
  // wave order.
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) {
    s_loss += __shfl_xor(s_loss, x, 64);
    s_gs += __shfl_xor(s_gs, x, 64);
    s_g += __shfl_xor(s_g, x, 64);
  }
  float* red = reinterpret_cast<float*>(lds + RED_OFF);
  if (lane == 0) {
    red[3 * wave + 0] = s_loss;
    red[3 * wave + 1] = s_gs;
    red[3 * wave + 2] = s_g;
  }
  __syncthreads();
  if (tid < 3)
    ws[((long long)tp.tm * tiles_n + tp.tn) * 3 + tid] =
        ((red[tid] + red[3 + tid]) + red[6 + tid]) + red[9 + tid];

  if (WRITE_G) store_g_tile(lds, g, ldg, m0, n0, b, n);
}

}  // namespace

extern "C" {

// Edge of the square output tile: the partials workspace holds
// ceil(b / tile)·ceil(n / tile) triples.
int sigmoid_distill_tile_dim() { return BM; }

// Sigmoid distillation loss over the (b, n) block of the student pair
// zimg (b, d) × ztxt (n, d) against the teacher pair timg (b, d_t) ×
// ttxt (n, d_t), all bf16 row-major contiguous, d and d_t positive multiples
// of 8; tprime, bias, tprime_t, bias_t: device fp32 scalars; 0 ≤ alpha ≤ 1
// weighs the teacher's probability against the hard label j == i + diag
// (diag == INT_MIN: no hard positive).  ws[tile] = (Σ term, Σ g·s, Σ g) per
// tile in row-major tile order.  g: null for the loss-only forward, otherwise
// a (b, n) bf16 view with row stride ldg elements.  Returns non-zero,
// launching nothing, on anything unsupported.
int sigmoid_distill_bf16(uintptr_t stream, const void* zimg, const void* ztxt,
                         const void* tprime, const void* bias,
                         const void* timg, const void* ttxt,
                         const void* tprime_t, const void* bias_t, void* g,
                         void* ws, int b, int n, int d, int d_t,
                         long long ldg, int diag, float alpha) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d) ||
      !pair_dims_ok(timg, ttxt, b, n, d_t) || tprime == nullptr ||
      bias == nullptr || tprime_t == nullptr || bias_t == nullptr ||
      ws == nullptr || !(alpha >= 0.f && alpha <= 1.f))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)tprime | (uintptr_t)bias | (uintptr_t)tprime_t |
       (uintptr_t)bias_t | (uintptr_t)ws) % 4 != 0 ||
      (uintptr_t)g % 2 != 0)
    return (int)hipErrorInvalidValue;
  if (g != nullptr && ldg < n) return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (!pair_grid_ok(tiles_m, tiles_n)) return (int)hipErrorInvalidValue;
  const auto kernel = g != nullptr ? sigmoid_distill_kernel<true>
                                   : sigmoid_distill_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(tiles_m * tiles_n), dim3(NTHREADS), 0,
                     (hipStream_t)stream, (const __bf16*)zimg,
                     (const __bf16*)ztxt, (const float*)tprime,
                     (const float*)bias, (const __bf16*)timg,
                     (const __bf16*)ttxt, (const float*)tprime_t,
                     (const float*)bias_t, (__bf16*)g, (float*)ws, b, n, d,
                     d_t, ldg, diag, alpha, tiles_m, tiles_n,
                     (const unsigned char*)nullptr,
                     (const unsigned char*)nullptr, 0);
  return (int)hipGetLastError();
}

// The same loss with an MXFP8 teacher pair: timg_q (b, d_t), ttxt_q (n, d_t)
// OCP e4m3fn bytes, row-major contiguous, d_t a multiple of 32; timg_e8 (b
// rows), ttxt_e8 (n rows) their e8m0 block scales, byte kb of a row for
// elements 32·kb … +31, 4-byte aligned with rows lde bytes apart, exactly
// 4·ceil(d_t / 128).  The teacher's dot is the true dot of the dequantised
// values (the MFMA applies the scales), so tprime_t and bias_t are those of
// sigmoid_distill_bf16.  The student pair, ws, g and every other check as
// there.  Returns non-zero, launching nothing, on anything unsupported.
int sigmoid_distill_mxt(uintptr_t stream, const void* zimg, const void* ztxt,
                        const void* tprime, const void* bias,
                        const void* timg_q, const void* timg_e8,
                        const void* ttxt_q, const void* ttxt_e8,
                        const void* tprime_t, const void* bias_t, void* g,
                        void* ws, int b, int n, int d, int d_t, long long lde,
                        long long ldg, int diag, float alpha) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d) ||
      !pair_dims_ok_mx(timg_q, timg_e8, ttxt_q, ttxt_e8, b, n, d_t, lde,
                       lde) ||
      tprime == nullptr || bias == nullptr || tprime_t == nullptr ||
      bias_t == nullptr || ws == nullptr || !(alpha >= 0.f && alpha <= 1.f))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)tprime | (uintptr_t)bias | (uintptr_t)tprime_t |
       (uintptr_t)bias_t | (uintptr_t)ws) % 4 != 0 ||
      (uintptr_t)g % 2 != 0)
    return (int)hipErrorInvalidValue;
  if (g != nullptr && ldg < n) return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (!pair_grid_ok(tiles_m, tiles_n)) return (int)hipErrorInvalidValue;
  const auto kernel = g != nullptr ? sigmoid_distill_kernel<true, mx_e4m3>
                                   : sigmoid_distill_kernel<false, mx_e4m3>;
  hipLaunchKernelGGL(kernel, dim3(tiles_m * tiles_n), dim3(NTHREADS), 0,
                     (hipStream_t)stream, (const __bf16*)zimg,
                     (const __bf16*)ztxt, (const float*)tprime,
                     (const float*)bias, (const mx_e4m3*)timg_q,
                     (const mx_e4m3*)ttxt_q, (const float*)tprime_t,
                     (const float*)bias_t, (__bf16*)g, (float*)ws, b, n, d,
                     d_t, ldg, diag, alpha, tiles_m, tiles_n,
                     (const unsigned char*)timg_e8,
                     (const unsigned char*)ttxt_e8, (int)lde);
  return (int)hipGetLastError();
}

}  // extern "C"
