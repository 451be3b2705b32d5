// The 128×128 pair tile shared by rank_kernels.hip, softmax_kernels.hip,
// topk_kernels.hip, idlabel_kernels.hip and softmax_id_kernels.hip (gfx950,
// MI355X): constants, the block walk, the main loop that leaves a tile of
// <zimg_i, ztxt_j> dot products in MFMA accumulators, and the helpers the
// epilogues share (the positive's column, the log-sum-exp guard, the sample-id
// staging, the g write-out).  Each
// including file adds its own epilogue and C entry points; nothing here is
// exported.  Everything sits in an anonymous namespace, so each translation
// unit gets its own copy.
//
// Tile.  128×128 output tile per 256-thread workgroup, 4 waves as
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
// Placement.  One workgroup per tile on a 1-D grid; the block id is remapped
// so consecutive logical ids share an XCD, and logical ids walk the tile grid
// in groups of 8 tile-rows, column by column, so the workgroups in flight on
// an XCD share operand panels in its L2.

#pragma once

#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
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
// g staging tile: 128 rows of 256 B, padded to 272 B (68 dwords ≡ 4 mod 64
// banks) so the 8-byte writes of lanes (row fr, quad fq) fall on distinct
// banks within each half-wave.
constexpr int G_PITCH = 2 * BN + 16;
constexpr int G_STAGE_BYTES = BM * G_PITCH;   // 34 KiB of the 64 KiB
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

inline int ceil_div(int a, int b) { return (a - 1) / b + 1; }  // a ≥ 1

// What every C entry checks of its embeddings: zimg (b, d) and ztxt (n, d)
// given and 16-byte aligned, a non-empty block, d a positive multiple of 8.
inline bool pair_dims_ok(const void* zimg, const void* ztxt, int b, int n,
                         int d) {
  if (zimg == nullptr || ztxt == nullptr) return false;
  if (b < 1 || n < 1 || d < 8 || d % 8 != 0) return false;
  return ((uintptr_t)zimg | (uintptr_t)ztxt) % 16 == 0;
}

// A 1-D grid of rows · cols workgroups stays below 2³¹ (the block walk is in
// int).
inline bool pair_grid_ok(int rows, int cols) {
  return (long long)rows * cols < (1ll << 31);
}

// Byte offset of 16-byte chunk `ch` (0..7) of row `row` in an operand slab.
__device__ __forceinline__ int lds_off(int row, int ch) {
  return ROW_BYTES * row + 16 * (ch ^ ((row >> 1) & 7));
}

// XCD-contiguous (bijective) remap of a 1-D grid of `nwg` workgroups: block
// ids go round-robin over the 8 XCDs, so XCD x is given the x-th contiguous
// run of logical ids.
__device__ __forceinline__ int xcd_logical_id(int nwg) {
  const int xcd = (int)(blockIdx.x & 7), slot = (int)(blockIdx.x >> 3);
  const int q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
}

struct TilePos { int tm, tn; };

// The remap, then the grouped column-major walk.
__device__ __forceinline__ TilePos tile_of_block(int tiles_m, int tiles_n) {
  const int lid = xcd_logical_id(tiles_m * tiles_n);
  const int per_group = GROUP_M * tiles_n;
  const int group = lid / per_group;
  const int first_m = group * GROUP_M;
  const int group_h = (tiles_m - first_m < GROUP_M) ? tiles_m - first_m
                                                    : GROUP_M;
  const int in_group = lid - group * per_group;
  return TilePos{first_m + in_group % group_h, in_group / group_h};
}

// The main loop: the tile's dot products, 0 where either row lies outside its
// matrix.  With wm = wave >> 1, wn = wave & 1:
//
// TEXT_FIRST (the MFMA operands exchanged, text fragment first): the
// accumulator holds the transposed 16×16 block, lane l owns image row (l & 15)
// and four consecutive text columns,
//   acc[i][j][r] = <zimg row m0 + wm·64 + i·16 + (lane & 15),
//                   ztxt row n0 + wn·64 + j·16 + 4·(lane >> 4) + r>.
// A lane's values are then contiguous in the output row, and a row reduction
// needs 2 shuffles where a column reduction needs 4.
//
// !TEXT_FIRST (the C layout of the 16×16 MFMA: col = lane & 15,
// row = (lane >> 4)·4 + reg):
//   acc[i][j][r] = <zimg row m0 + wm·64 + i·16 + 4·(lane >> 4) + r,
//                   ztxt row n0 + wn·64 + j·16 + (lane & 15)>.
//
// `lds` holds at least 2 · BUF_BYTES bytes, 16-byte aligned.  Ends on a
// barrier: every read of the staging buffers has retired, the caller may
// reuse `lds`.
template <bool TEXT_FIRST>
__device__ __forceinline__ void pair_tile_dots(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt, int b,
    int n, int d, int m0, int n0, unsigned char* lds, f32x4 (&acc)[4][4]) {
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
              TEXT_FIRST ? bfr[j] : af[i], TEXT_FIRST ? af[i] : bfr[j],
              acc[i][j], 0, 0, 0);
    }

    if (more) store_step((s + 1) & 1);
    __syncthreads();
  }
}

// Column of row `row`'s positive, j == row + diag; −1 when there is none in
// the block (diag == DIAG_NONE, or the column falls outside [0, n)).
__device__ __forceinline__ int positive_col(int row, int diag, int n) {
  const long long pos = (long long)row + diag;
  return (diag != DIAG_NONE && pos >= 0 && pos < n) ? (int)pos : -1;
}

// The max subtracted in the exp(x − m) terms of a log-sum-exp: m == −inf
// (nothing valid) is replaced by 0 so that the difference stays −inf instead
// of becoming NaN.
__device__ __forceinline__ float safe_max(float m) {
  return m == -__builtin_inff() ? 0.f : m;
}

// Sample ids (idlabel_kernels.hip, softmax_id_kernels.hip).  Stage the tile's
// ids in the IDS_BYTES at `idl`: threads 0..127 a row id, 128..255 a column
// id; −1 outside the block, so padding is masked by the same test as a
// negative id.  Ends on a barrier.
constexpr int IDS_BYTES = (BM + BN) * 8;      // 2 KiB

__device__ __forceinline__ void stage_ids(long long* idl,
                                          const long long* __restrict__ img_ids,
                                          const long long* __restrict__ txt_ids,
                                          int m0, int n0, int b, int n) {
  const int tid = threadIdx.x;
  const bool is_row = tid < BM;
  const int e = is_row ? m0 + tid : n0 + (tid - BM);
  const int len = is_row ? b : n;
  const long long* src = is_row ? img_ids : txt_ids;
  long long id = -1;
  if (e < len) id = src[e];
  idl[tid] = id;
  __syncthreads();
}

// The four column ids of fragment column lcol0 … +3.
__device__ __forceinline__ void load_col_ids(const long long* idl, int lcol0,
                                             long long (&cid)[4]) {
  const longlong2 c01 = *reinterpret_cast<const longlong2*>(idl + BM + lcol0);
  const longlong2 c23 =
      *reinterpret_cast<const longlong2*>(idl + BM + lcol0 + 2);
  cid[0] = c01.x; cid[1] = c01.y; cid[2] = c23.x; cid[3] = c23.y;
}

// Write-out of the bf16 g tile staged in `lds` ([BM] rows at G_PITCH bytes)
// into the (b, n) view `g` of row stride ldg: 16 threads cover one 256-byte
// tile row.  A 16-byte store where the segment is whole and its address
// aligned, 2-byte stores otherwise (ragged edge, odd row stride or column
// offset).  The caller's barrier orders the staging writes before this.
__device__ __forceinline__ void store_g_tile(const unsigned char* lds,
                                             __bf16* __restrict__ g,
                                             long long ldg, int m0, int n0,
                                             int b, int n) {
  const int tid = threadIdx.x;
  const int ch = tid & 15;
#pragma unroll
  for (int k = 0; k < BM / 16; ++k) {
    const int lrow = (tid >> 4) + 16 * k;
    const int row = m0 + lrow, col = n0 + ch * 8;
    if (row >= b || col >= n) continue;
    const uint4 v =
        *reinterpret_cast<const uint4*>(lds + lrow * G_PITCH + 16 * ch);
    __bf16* dst = g + (long long)row * ldg + col;
    if (col + 8 <= n && ((uintptr_t)dst & 15) == 0) {
      *reinterpret_cast<uint4*>(dst) = v;
    } else {
      const unsigned short* h = reinterpret_cast<const unsigned short*>(&v);
      unsigned short* dst16 = reinterpret_cast<unsigned short*>(dst);
#pragma unroll
      for (int x = 0; x < 8; ++x)
        if (col + x < n) dst16[x] = h[x];
    }
  }
}

}  // namespace
