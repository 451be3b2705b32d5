// Fused softmax (InfoNCE / CLIP) contrastive loss for gfx950 (MI355X): the
// log-sum-exp of every row and every column of the image×text logit grid,
// and the dL/dlogit slab of the backward pass, without the grid ever
// reaching memory in fp32.
//
//   z_ij      = t · <zimg_i, ztxt_j>,  t = exp(t')     zimg (b, d), ztxt (n, d)
//   row_lse_i = log Σ_j exp(z_ij)      col_lse_j = log Σ_i exp(z_ij)
//   g_ij      = row_w_i·exp(z_ij − row_lse_i) + col_w_j·exp(z_ij − col_lse_j)
//               − [j == i + diag]·(row_w_i + col_w_j)
//
// Three kernels:
//
// - softmax_lse_partials_kernel: per 128×128 tile, each row's
//   (max, Σ exp(z − max)) over the tile's columns and each column's over the
//   tile's rows, written as float2 pairs to workspaces laid out (tiles_n, b)
//   and (tiles_m, n).  `max` is in units of z; the positive is not masked.
// - softmax_lse_finish_kernel: one thread per row / column folds its tile
//   partials in tile order: lse = M + log Σ_t sum_t·exp(max_t − M).
// - softmax_g_kernel: the same main loop; the epilogue evaluates g from the
//   fp32 LSE and weight vectors, stages the bf16 tile in LDS and writes it as
//   coalesced 16-byte row segments into a (b, n) view of row stride ldg, and
//   leaves one fp32 partial Σ g_ij·s_ij (s = z / t) per tile.
//
// There is no floating-point atomic anywhere: every reduction has a fixed
// order, so all results are bitwise reproducible.
//
// Structure.  The tile, its main loop (text fragment first: lane l owns image
// row (l & 15) and four consecutive text columns of each fragment, so its g
// values are one 8-byte LDS write per fragment), the block walk and the g
// write-out are pair_tile.h's; this file adds the epilogues.
//
// Padding.  A zero-filled padding column scores z = 0, which would dominate a
// row of negative logits: every element outside the block is replaced by
// −inf before a reduction.  A partial over padding alone is (−inf, 0); the
// subtraction of the max is guarded so that it never forms inf − inf.
//
// exp / log are the bare v_exp_f32 / v_log_f32 (base 2) with the ln 2 factors
// folded into the scale of the argument and of the result.

#include "pair_tile.h"

namespace {

static_assert(G_STAGE_BYTES + 16 <= 2 * BUF_BYTES, "g staging exceeds LDS");

// exp(x − m) terms of a log-sum-exp in base 2: `sc2` is t·log2 e, `m` a raw
// dot product, guarded by pair_tile.h's safe_max.
__launch_bounds__(NTHREADS) __global__ void softmax_lse_partials_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, float2* __restrict__ row_ws,
    float2* __restrict__ col_ws, int b, int n, int d, int tiles_m,
    int tiles_n) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];
  static_assert(sizeof(lds) >= 2 * BUF_BYTES, "staging buffers exceed the LDS");

  const TilePos tp = tile_of_block(tiles_m, tiles_n);
  const int m0 = tp.tm * BM, n0 = tp.tn * BN;
  f32x4 acc[4][4];
  pair_tile_dots<true>(zimg, ztxt, b, n, d, m0, n0, lds, acc);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const float inf = __builtin_inff();
  const float t = expf(tprime[0]);
  const float sc2 = t * LOG2E;
  const bool rows_on = row_ws != nullptr;
  const bool cols_on = col_ws != nullptr;

  // Everything outside the block becomes −inf.
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool row_ok = m0 + wm * 64 + i * 16 + fr < b;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool col_ok = n0 + wn * 64 + j * 16 + fq * 4 + r < n;
        if (!(row_ok && col_ok)) acc[i][j][r] = -inf;
      }
  }

  // part_row[wn][128], part_col[wm][128] as (max of raw dots, sum) pairs.
  float2* part_row = reinterpret_cast<float2*>(lds);
  float2* part_col = part_row + 2 * BM;

  if (rows_on) {
    // A row lives in the 4 lanes that share fr (lane bits 4-5).
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float m = -inf;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, acc[i][j][r]);
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      const float ms = safe_max(m);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          s += __builtin_amdgcn_exp2f((acc[i][j][r] - ms) * sc2);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (fq == 0) part_row[wn * BM + wm * 64 + i * 16 + fr] = float2{m, s};
    }
  }
  if (cols_on) {
    // A column lives in the 16 lanes that share fq (lane bits 0-3).
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = fmaxf(fmaxf(acc[0][j][r], acc[1][j][r]),
                        fmaxf(acc[2][j][r], acc[3][j][r]));
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) m = fmaxf(m, __shfl_xor(m, x, 64));
        const float ms = safe_max(m);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          s += __builtin_amdgcn_exp2f((acc[i][j][r] - ms) * sc2);
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) s += __shfl_xor(s, x, 64);
        if (fr == 0)
          part_col[wm * BN + wn * 64 + j * 16 + fq * 4 + r] = float2{m, s};
      }
  }
  __syncthreads();

  // Fold the two waves of each row / column (wave 0 first) and store.
  const bool row_half = tid < BM;
  const int e = row_half ? tid : tid - BM;
  if (row_half ? !rows_on : !cols_on) return;
  const float2* part = row_half ? part_row : part_col;
  const float2 p0 = part[e], p1 = part[BM + e];
  const float m = fmaxf(p0.x, p1.x);
  const float ms = safe_max(m);
  const float s = p0.y * __builtin_amdgcn_exp2f((p0.x - ms) * sc2) +
                  p1.y * __builtin_amdgcn_exp2f((p1.x - ms) * sc2);
  if (row_half) {
    if (m0 + e < b)
      row_ws[(long long)tp.tn * b + (m0 + e)] = float2{m * t, s};
  } else {
    if (n0 + e < n)
      col_ws[(long long)tp.tm * n + (n0 + e)] = float2{m * t, s};
  }
}

// One thread per row (ids 0 … b−1, when row_lse is given) or column (the
// ids after them): fold `tiles` partials, tile 0 first.
__launch_bounds__(NTHREADS) __global__ void softmax_lse_finish_kernel(
    const float2* __restrict__ row_ws, const float2* __restrict__ col_ws,
    float* __restrict__ row_lse, float* __restrict__ col_lse, int b, int n,
    int tiles_m, int tiles_n) {
  const long long id = (long long)blockIdx.x * NTHREADS + threadIdx.x;
  const long long nrows = row_lse != nullptr ? b : 0;
  const long long ncols = col_lse != nullptr ? n : 0;
  const float2* ws;
  float* out;
  long long len, e;
  int tiles;
  if (id < nrows) {
    ws = row_ws; out = row_lse; len = b; e = id; tiles = tiles_n;
  } else if (id - nrows < ncols) {
    ws = col_ws; out = col_lse; len = n; e = id - nrows; tiles = tiles_m;
  } else {
    return;
  }
  float m = -__builtin_inff();
  for (int k = 0; k < tiles; ++k) m = fmaxf(m, ws[k * len + e].x);
  const float ms = safe_max(m);
  float s = 0.f;
  for (int k = 0; k < tiles; ++k) {
    const float2 p = ws[k * len + e];
    s += p.y * __builtin_amdgcn_exp2f((p.x - ms) * LOG2E);
  }
  out[e] = m + LN2 * __builtin_amdgcn_logf(s);
}

__launch_bounds__(NTHREADS) __global__ void softmax_g_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const float* __restrict__ row_lse,
    const float* __restrict__ row_w, const float* __restrict__ col_lse,
    const float* __restrict__ col_w, __bf16* __restrict__ g,
    float* __restrict__ gs_ws, int b, int n, int d, long long ldg, int diag,
    int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];
  static_assert(sizeof(lds) >= 2 * BUF_BYTES, "staging buffers exceed the LDS");

  const TilePos tp = tile_of_block(tiles_m, tiles_n);
  const int m0 = tp.tm * BM, n0 = tp.tn * BN;
  f32x4 acc[4][4];
  pair_tile_dots<true>(zimg, ztxt, b, n, d, m0, n0, lds, acc);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const float sc2 = expf(tprime[0]) * LOG2E;
  const bool rows_on = row_lse != nullptr;
  const bool cols_on = col_lse != nullptr;

  // Per column of this lane: −col_lse·log2 e and col_w (0 outside the block).
  float cl2[4][4], cw[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = n0 + wn * 64 + j * 16 + fq * 4 + r;
      const bool on = cols_on && col < n;
      cl2[j][r] = on ? -col_lse[col] * LOG2E : 0.f;
      cw[j][r] = on ? col_w[col] : 0.f;
    }

  float s_gs = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lrow = wm * 64 + i * 16 + fr;
    const int row = m0 + lrow;
    const bool row_ok = row < b;
    const float rl2 = (rows_on && row_ok) ? -row_lse[row] * LOG2E : 0.f;
    const float rw = (rows_on && row_ok) ? row_w[row] : 0.f;
    const int pc = positive_col(row, diag, n);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col0 = n0 + wn * 64 + j * 16 + fq * 4;
      bf16x4 out;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[i][j][r];
        // A skipped side adds no term at all (never 0 · exp(…)).
        float gv = 0.f;
        if (rows_on)
          gv += rw * __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, rl2));
        if (cols_on)
          gv += cw[j][r] * __builtin_amdgcn_exp2f(
                    __builtin_fmaf(s, sc2, cl2[j][r]));
        if (col0 + r == pc) gv -= rw + cw[j][r];
        if (!(row_ok && col0 + r < n)) gv = 0.f;
        s_gs += gv * s;
        out[r] = (__bf16)gv;
      }
      *reinterpret_cast<bf16x4*>(lds + lrow * G_PITCH
                                 + 2 * (wn * 64 + j * 16 + fq * 4)) = out;
    }
  }

  // Σ g·s of the tile: lanes by xor shuffles, then the four waves in order.
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) s_gs += __shfl_xor(s_gs, x, 64);
  float* red = reinterpret_cast<float*>(lds + G_STAGE_BYTES);
  if (lane == 0) red[wave] = s_gs;
  __syncthreads();
  if (tid == 0)
    gs_ws[(long long)tp.tm * tiles_n + tp.tn] =
        ((red[0] + red[1]) + red[2]) + red[3];

  store_g_tile(lds, g, ldg, m0, n0, b, n);
}

// The embedding checks plus what both entries add: t' and the grid size.
bool dims_ok(const void* zimg, const void* ztxt, const void* tprime, int b,
             int n, int d) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d) || tprime == nullptr ||
      (uintptr_t)tprime % 4 != 0)
    return false;
  return pair_grid_ok(ceil_div(b, BM), ceil_div(n, BN));
}

}  // namespace

extern "C" {

// Edge of the square output tile: workspaces are sized by ceil(b / tile) and
// ceil(n / tile).
int softmax_tile_dim() { return BM; }

// row_lse[i] = log Σ_j exp(z_ij), col_lse[j] = log Σ_i exp(z_ij) over the
// (b, n) block of zimg (b, d) × ztxt (n, d), bf16 row-major contiguous, with
// z = exp(*tprime)·<·,·> (tprime: device fp32).  row_ws / col_ws are float2
// workspaces of ceil(n/128)·b and ceil(b/128)·n pairs.  A side whose
// workspace and output are both null is skipped.  Returns non-zero,
// launching nothing, on anything unsupported.
int softmax_lse_bf16(uintptr_t stream, const void* zimg, const void* ztxt,
                     const void* tprime, void* row_ws, void* col_ws,
                     void* row_lse, void* col_lse, int b, int n, int d) {
  if (!dims_ok(zimg, ztxt, tprime, b, n, d))
    return (int)hipErrorInvalidValue;
  if ((row_ws == nullptr) != (row_lse == nullptr) ||
      (col_ws == nullptr) != (col_lse == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)row_ws | (uintptr_t)col_ws) % 8 != 0 ||
      ((uintptr_t)row_lse | (uintptr_t)col_lse) % 4 != 0)
    return (int)hipErrorInvalidValue;
  if (row_lse == nullptr && col_lse == nullptr) return 0;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  hipLaunchKernelGGL(softmax_lse_partials_kernel, dim3(tiles_m * tiles_n),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt,
                     (const float*)tprime, (float2*)row_ws, (float2*)col_ws,
                     b, n, d, tiles_m, tiles_n);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  const long long ids = (row_lse != nullptr ? (long long)b : 0) +
                        (col_lse != nullptr ? (long long)n : 0);
  hipLaunchKernelGGL(softmax_lse_finish_kernel,
                     dim3((unsigned)((ids + NTHREADS - 1) / NTHREADS)),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const float2*)row_ws, (const float2*)col_ws,
                     (float*)row_lse, (float*)col_lse, b, n, tiles_m,
                     tiles_n);
  return (int)hipGetLastError();
}

// g (b, n) bf16 with row stride ldg elements, and gs_ws[tile] = Σ g_ij·s_ij
// over each of the ceil(b/128)·ceil(n/128) tiles (row-major tile order).
// A side whose lse and weight pointers are both null contributes nothing;
// diag == INT_MIN: no positives.
int softmax_g_bf16(uintptr_t stream, const void* zimg, const void* ztxt,
                   const void* tprime, const void* row_lse, const void* row_w,
                   const void* col_lse, const void* col_w, void* g,
                   void* gs_ws, int b, int n, int d, long long ldg,
                   int diag) {
  if (!dims_ok(zimg, ztxt, tprime, b, n, d) || g == nullptr ||
      gs_ws == nullptr || ldg < n)
    return (int)hipErrorInvalidValue;
  if ((row_lse == nullptr) != (row_w == nullptr) ||
      (col_lse == nullptr) != (col_w == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)row_lse | (uintptr_t)row_w | (uintptr_t)col_lse |
       (uintptr_t)col_w | (uintptr_t)gs_ws) % 4 != 0 ||
      (uintptr_t)g % 2 != 0)
    return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  hipLaunchKernelGGL(softmax_g_kernel, dim3(tiles_m * tiles_n),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt,
                     (const float*)tprime, (const float*)row_lse,
                     (const float*)row_w, (const float*)col_lse,
                     (const float*)col_w, (__bf16*)g, (float*)gs_ws, b, n, d,
                     ldg, diag, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

}  // extern "C"
