// Fused retrieval rank counts for gfx950 (MI355X): a second reduction over
// the image×text pair grid, next to the loss kernels' scalar one.
//
//   s_ij       = <zimg_i, ztxt_j>          zimg (b, d), ztxt (n, d) bf16
//   row_cnt[i] += #{ j : s_ij > row_thr[i] }
//   col_cnt[j] += #{ i : s_ij > col_thr[j] }
//
// Both counts skip the positive pair j == i + diag (diag = INT_MIN: none) and
// everything a ragged tile pads.  With the thresholds set to the positive
// pair's own score the counts are the retrieval ranks (losses/retrieval.py);
// the (b, n) logits never leave the MFMA accumulators.  The counts are int32
// and ADDED into the caller's buffers, so column chunks, several calls and
// several ranks compose by integer addition: the result does not depend on
// the order of anything and is bitwise reproducible.
//
// Structure.  The tile, its main loop (image fragment first: the plain MFMA
// C layout) and the block walk are pair_tile.h's; this file adds the epilogue.
//
// Epilogue.  An element outside the block or on the positive diagonal is
// replaced by −inf, which exceeds no threshold (a zero-filled padding column
// scores 0 and would otherwise beat every negative threshold).  A lane packs
// its counts as bytes (at most 4 per row and 16 per column per lane, 64 after
// the wave reduction), combines them across the 16 lanes that share a row
// (4 shuffles) or the 4 lane groups that share a column (2 shuffles), and
// each wave leaves its 64 row and 64 column sums in its own LDS slot.  The
// workgroup then adds the two waves of each row / column and issues one
// integer atomicAdd per row and per column of the tile.  Counts never pass
// through floating point.

#include "pair_tile.h"

namespace {

__launch_bounds__(NTHREADS) __global__ void pair_rank_counts_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ row_thr, const float* __restrict__ col_thr,
    int* __restrict__ row_cnt, int* __restrict__ col_cnt, int b, int n, int d,
    int diag, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];
  static_assert(sizeof(lds) >= 2 * BUF_BYTES, "staging buffers exceed the LDS");

  const TilePos tp = tile_of_block(tiles_m, tiles_n);
  const int m0 = tp.tm * BM, n0 = tp.tn * BN;
  f32x4 acc[4][4];
  pair_tile_dots<false>(zimg, ztxt, b, n, d, m0, n0, lds, acc);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;

  // C layout of the 16×16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg.
  const float inf = __builtin_inff();
  const bool rows_on = row_thr != nullptr;
  const bool cols_on = col_thr != nullptr;

  int col[4];
  bool col_ok[4];
  float ct[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    col[j] = n0 + wn * 64 + j * 16 + fr;
    col_ok[j] = col[j] < n;
    ct[j] = (cols_on && col_ok[j]) ? col_thr[col[j]] : inf;
  }

  int rpack[4];                  // byte r: count of row i·16 + fq·4 + r
  int cc[4] = {0, 0, 0, 0};      // count of column j
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    rpack[i] = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wm * 64 + i * 16 + fq * 4 + r;
      const bool row_ok = row < b;
      const float rt = (rows_on && row_ok) ? row_thr[row] : inf;
      const int pc = positive_col(row, diag, n);
      int rc = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = row_ok && col_ok[j] && col[j] != pc;
        const float s = ok ? acc[i][j][r] : -inf;
        rc += (s > rt) ? 1 : 0;
        cc[j] += (s > ct[j]) ? 1 : 0;
      }
      rpack[i] |= rc << (8 * r);
    }
  }
  int cpack = cc[0] | (cc[1] << 8) | (cc[2] << 16) | (cc[3] << 24);

  // Rows: sum over the 16 lanes of a group (lane bits 0-3); columns: over
  // the 4 groups (lane bits 4-5).  Bytes stay ≤ 64, so no carry crosses.
#pragma unroll
  for (int m = 1; m < 16; m <<= 1)
#pragma unroll
    for (int i = 0; i < 4; ++i) rpack[i] += __shfl_xor(rpack[i], m, 64);
  cpack += __shfl_xor(cpack, 16, 64);
  cpack += __shfl_xor(cpack, 32, 64);

  // The k-loop's last barrier has retired every read of the staging buffers:
  // reuse them as part[0][wn][128] (rows) and part[1][wm][128] (columns).
  int* part = reinterpret_cast<int*>(lds);
  if (fr == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        part[wn * 128 + wm * 64 + i * 16 + fq * 4 + r] =
            (rpack[i] >> (8 * r)) & 0xff;
  }
  if (fq == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      part[256 + wm * 128 + wn * 64 + j * 16 + fr] = (cpack >> (8 * j)) & 0xff;
  }
  __syncthreads();

  if (tid < 128) {
    const int v = part[tid] + part[128 + tid];
    if (rows_on && v != 0 && m0 + tid < b) atomicAdd(row_cnt + m0 + tid, v);
  } else {
    const int t = tid - 128;
    const int v = part[256 + t] + part[384 + t];
    if (cols_on && v != 0 && n0 + t < n) atomicAdd(col_cnt + n0 + t, v);
  }
}

}  // namespace

extern "C" {

// row_cnt[i] += #{j : s_ij > row_thr[i]}, col_cnt[j] += #{i : s_ij >
// col_thr[j]} over the (b, n) block of zimg (b, d) × ztxt (n, d), bf16
// row-major contiguous, skipping j == i + diag (INT_MIN: no positives).  A
// side whose threshold and count pointers are both null is skipped.  Returns
// non-zero, launching nothing, on anything unsupported: null embeddings, a
// half-given side, d not a positive multiple of 8, misaligned pointers.
int pair_rank_counts_bf16(uintptr_t stream, const void* zimg,
                          const void* ztxt, const void* row_thr,
                          const void* col_thr, void* row_cnt, void* col_cnt,
                          int b, int n, int d, int diag) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d)) return (int)hipErrorInvalidValue;
  if ((row_thr == nullptr) != (row_cnt == nullptr) ||
      (col_thr == nullptr) != (col_cnt == nullptr))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)row_thr | (uintptr_t)col_thr | (uintptr_t)row_cnt |
       (uintptr_t)col_cnt) % 4 != 0)
    return (int)hipErrorInvalidValue;
  if (row_thr == nullptr && col_thr == nullptr) return 0;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (!pair_grid_ok(tiles_m, tiles_n)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pair_rank_counts_kernel, dim3(tiles_m * tiles_n),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt,
                     (const float*)row_thr, (const float*)col_thr,
                     (int*)row_cnt, (int*)col_cnt, b, n, d, diag, tiles_m,
                     tiles_n);
  return (int)hipGetLastError();
}

}  // extern "C"
