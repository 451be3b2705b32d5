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
// Structure.  128×128 output tile per 256-thread workgroup, 4 waves as
// 2 (M) × 2 (N), 64×64 (4×4 fragments of v_mfma_f32_16x16x32_bf16) each,
// fp32 accumulation.  Both operands are K-contiguous, so a k-step stages a
// [128 rows][64 k] slab of each in LDS (double-buffered, 2 × 32 KiB) through
// registers with 16-byte loads — rows past b / n and k past d are zero-filled,
// so one kernel serves interior and ragged tiles — and a lane's fragment is
// one ds_read_b128.  The 16-byte chunk index is XOR-ed with (row >> 1) & 7:
// the 16 rows of a fragment read land on the 16 distinct 16-byte slots of the
// 256-byte bank row.  Two workgroups (64 KiB each) share a CU and hide each
// other's staging.
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
//
// Placement.  One workgroup per tile on a 1-D grid; the block id is remapped
// so consecutive logical ids share an XCD, and logical ids walk the tile grid
// in groups of 8 tile-rows, column by column, so the workgroups in flight on
// an XCD share operand panels in its L2.

#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BM = 128;          // image rows per tile
constexpr int BN = 128;          // text rows (logit columns) per tile
constexpr int BK = 64;           // k per step: one 128-byte LDS row
constexpr int NTHREADS = 256;    // 4 waves as 2 (M) × 2 (N), 64×64 each
constexpr int ROW_BYTES = 2 * BK;
constexpr int OP_BYTES = BM * ROW_BYTES;      // one operand slab: 16 KiB
constexpr int BUF_BYTES = 2 * OP_BYTES;       // zimg slab + ztxt slab
constexpr int LOADS = BM * 8 / NTHREADS;      // 16-B chunks per thread: 4
constexpr int GROUP_M = 8;       // tile-rows per locality group
constexpr int DIAG_NONE = INT_MIN;

inline int ceil_div(int a, int b) { return (a - 1) / b + 1; }  // a ≥ 1

// Byte offset of 16-byte chunk `ch` (0..7) of row `row` in an operand slab.
__device__ __forceinline__ int lds_off(int row, int ch) {
  return ROW_BYTES * row + 16 * (ch ^ ((row >> 1) & 7));
}

__launch_bounds__(NTHREADS) __global__ void pair_rank_counts_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ row_thr, const float* __restrict__ col_thr,
    int* __restrict__ row_cnt, int* __restrict__ col_cnt, int b, int n, int d,
    int diag, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];

  // XCD-contiguous (bijective) remap, then the grouped column-major walk.
  const int nwg = tiles_m * tiles_n;
  const int xcd = (int)(blockIdx.x & 7), slot = (int)(blockIdx.x >> 3);
  const int q8 = nwg >> 3, r8 = nwg & 7;
  const int lid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8)
                  + slot;
  const int per_group = GROUP_M * tiles_n;
  const int group = lid / per_group;
  const int first_m = group * GROUP_M;
  const int group_h = (tiles_m - first_m < GROUP_M) ? tiles_m - first_m
                                                    : GROUP_M;
  const int in_group = lid - group * per_group;
  const int m0 = (first_m + in_group % group_h) * BM;
  const int n0 = (in_group / group_h) * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // Staging: thread t owns chunk t&7 of rows (t>>3) + 32·i, i = 0..3.
  const int ld_ch = tid & 7;
  const int ld_row = tid >> 3;
  const __bf16* a_src[LOADS];
  const __bf16* b_src[LOADS];
  bool a_ok[LOADS], b_ok[LOADS];
  int st_off[LOADS];
#pragma unroll
  for (int i = 0; i < LOADS; ++i) {
    const int row = ld_row + 32 * i;
    a_ok[i] = m0 + row < b;
    b_ok[i] = n0 + row < n;
    a_src[i] = zimg + (long long)(m0 + row) * d + ld_ch * 8;
    b_src[i] = ztxt + (long long)(n0 + row) * d + ld_ch * 8;
    st_off[i] = lds_off(row, ld_ch);
  }

  // Fragment reads: lane l takes row (l & 15), k = 8·(l >> 4) … +7 of each
  // 32-deep MFMA step, i.e. chunk 4·kk + (l >> 4).
  const int fr = lane & 15, fq = lane >> 4;
  int a_off[4][2], b_off[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      a_off[f][kk] = lds_off(wm * 64 + f * 16 + fr, 4 * kk + fq);
      b_off[f][kk] = OP_BYTES + lds_off(wn * 64 + f * 16 + fr, 4 * kk + fq);
    }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 ra[LOADS], rb[LOADS];

  auto load_step = [&](int s) {
    const int k0 = s * BK;
    const bool k_ok = k0 + ld_ch * 8 < d;     // d % 8 == 0: all or nothing
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      ra[i] = uint4{0u, 0u, 0u, 0u};
      rb[i] = uint4{0u, 0u, 0u, 0u};
      if (k_ok && a_ok[i])
        ra[i] = *reinterpret_cast<const uint4*>(a_src[i] + k0);
      if (k_ok && b_ok[i])
        rb[i] = *reinterpret_cast<const uint4*>(b_src[i] + k0);
    }
  };
  auto store_step = [&](int buf) {
    unsigned char* base = lds + buf * BUF_BYTES;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      *reinterpret_cast<uint4*>(base + st_off[i]) = ra[i];
      *reinterpret_cast<uint4*>(base + OP_BYTES + st_off[i]) = rb[i];
    }
  };

  const int nsteps = (d + BK - 1) / BK;
  load_step(0);
  store_step(0);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;
    if (more) load_step(s + 1);

    const unsigned char* base = lds + (s & 1) * BUF_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        af[f] = *reinterpret_cast<const bf16x8*>(base + a_off[f][kk]);
        bfr[f] = *reinterpret_cast<const bf16x8*>(base + b_off[f][kk]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], bfr[j], acc[i][j], 0, 0, 0);
    }

    if (more) store_step((s + 1) & 1);
    __syncthreads();
  }

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
      // Column of this row's positive, −1 when there is none in the block.
      const long long pos = (long long)row + diag;
      const int pc = (diag != DIAG_NONE && pos >= 0 && pos < n) ? (int)pos
                                                                : -1;
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
  if (zimg == nullptr || ztxt == nullptr) return (int)hipErrorInvalidValue;
  if ((row_thr == nullptr) != (row_cnt == nullptr) ||
      (col_thr == nullptr) != (col_cnt == nullptr))
    return (int)hipErrorInvalidValue;
  if (b < 1 || n < 1 || d < 8 || d % 8 != 0)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)zimg | (uintptr_t)ztxt) % 16 != 0 ||
      ((uintptr_t)row_thr | (uintptr_t)col_thr | (uintptr_t)row_cnt |
       (uintptr_t)col_cnt) % 4 != 0)
    return (int)hipErrorInvalidValue;
  if (row_thr == nullptr && col_thr == nullptr) return 0;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if ((long long)tiles_m * tiles_n >= (1ll << 31))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pair_rank_counts_kernel, dim3(tiles_m * tiles_n),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt,
                     (const float*)row_thr, (const float*)col_thr,
                     (int*)row_cnt, (int*)col_cnt, b, n, d, diag, tiles_m,
                     tiles_n);
  return (int)hipGetLastError();
}

}  // extern "C"
