// The 128×128 pair tile shared by rank_kernels.hip, softmax_kernels.hip,
// topk_kernels.hip, idlabel_kernels.hip, softmax_id_kernels.hip and
// rank_id_kernels.hip (gfx950, MI355X): constants, the block walk, the main
// loop that leaves a tile of <zimg_i, ztxt_j> dot products in MFMA
// accumulators, and the helpers the epilogues share (the positive's column,
// the log-sum-exp guard, the sample-id staging, the g write-out in bf16 and
// as an e4m3 slab pair).  Each
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
// e4m3 operands (pair_tile_dots_e4m3; idlabel_kernels.hip is its first user).
// The same tile, waves and accumulator layouts with one byte per element: a
// k-step is 128 elements, so the slab is byte for byte the bf16 one —
// [128 rows][128 B] per operand, the same staging thread map, lds_off and
// swizzle — and a step carries twice the k for the same bytes moved, the same
// LDS traffic and one barrier.  A fragment is one
// v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (per-tensor scales
// are the caller's, folded into its temperature): lane l supplies row l & 15
// and the 32-byte K-block l >> 4, chunks 2·(l >> 4) and 2·(l >> 4) + 1 of its
// row, two ds_read_b128.  Each of the two reads takes one fixed chunk index
// over the 16 rows of a fragment, which is the bf16 read pattern: the XOR with
// (row >> 1) & 7 gives 8 distinct slots over the 8 row pairs and the row
// parity picks the 128-byte half, 16 distinct 16-byte slots of the 256-byte
// bank row.  A fragment is 8 VGPRs, so the loop keeps the four text fragments
// of a step and streams the image fragments one at a time (40 VGPRs of
// fragments, not 64).
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
typedef __attribute__((ext_vector_type(8))) int i32x8;

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

// The same for e4m3 embeddings (one byte per element): d a positive multiple
// of 16, so that a row is a whole number of aligned 16-byte chunks.
inline bool pair_dims_ok_e4m3(const void* zimg_q, const void* ztxt_q, int b,
                              int n, int d) {
  if (zimg_q == nullptr || ztxt_q == nullptr) return false;
  if (b < 1 || n < 1 || d < 16 || d % 16 != 0) return false;
  return ((uintptr_t)zimg_q | (uintptr_t)ztxt_q) % 16 == 0;
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

// The main loop for e4m3 operands: zimg_q (b, d) and ztxt_q (n, d) are OCP
// e4m3fn bytes, row-major contiguous, d % 16 == 0 (pair_dims_ok_e4m3).  The
// contract of pair_tile_dots: the same acc layouts for both values of
// TEXT_FIRST, rows past b / n and k past d zero-filled (byte 0x00 is +0),
// 64-bit byte offsets, the same `lds`, and it ends on a barrier.  acc holds
// the raw dots of the e4m3 values: the MFMA runs with unit block scales and
// the caller folds its per-tensor scales into what it multiplies the dot by.
//
// A k-step is BK8 = 128 elements, one 128-byte LDS row, so staging is the
// bf16 code with 16 elements per chunk.  Per step a lane reads chunks 2·fq and
// 2·fq + 1 of its fragment row (the K-block the MFMA takes from lane group
// fq; both operands use the same map, so every product pairs equal k), keeps
// the four text fragments and streams the image fragments: 16 MFMAs of
// 16×16×128 per wave and step against 32 of 16×16×32 per 64 k for bf16.
constexpr int BK8 = ROW_BYTES;   // e4m3 k per step: one 128-byte LDS row
constexpr int MX_UNIT_SCALE = 0x7f7f7f7f;   // e8m0 127 = 2⁰ in every byte

template <bool TEXT_FIRST>
__device__ __forceinline__ void pair_tile_dots_e4m3(
    const unsigned char* __restrict__ zimg_q,
    const unsigned char* __restrict__ ztxt_q, int b, int n, int d, int m0,
    int n0, unsigned char* lds, f32x4 (&acc)[4][4]) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // Staging: thread t owns chunk t&7 of rows (t>>3) + 32·i, i = 0..3.
  const int ld_ch = tid & 7;
  const int ld_row = tid >> 3;
  const unsigned char* a_src[LOADS];
  const unsigned char* b_src[LOADS];
  bool a_ok[LOADS], b_ok[LOADS];
  int st_off[LOADS];
#pragma unroll
  for (int i = 0; i < LOADS; ++i) {
    const int row = ld_row + 32 * i;
    a_ok[i] = m0 + row < b;
    b_ok[i] = n0 + row < n;
    a_src[i] = zimg_q + (long long)(m0 + row) * d + ld_ch * 16;
    b_src[i] = ztxt_q + (long long)(n0 + row) * d + ld_ch * 16;
    st_off[i] = lds_off(row, ld_ch);
  }

  // Fragment reads: lane l takes row (l & 15), k = 32·(l >> 4) … +31 of the
  // 128-deep MFMA step, i.e. chunks 2·(l >> 4) and 2·(l >> 4) + 1.
  const int fr = lane & 15, fq = lane >> 4;
  int a_off[4][2], b_off[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      a_off[f][h] = lds_off(wm * 64 + f * 16 + fr, 2 * fq + h);
      b_off[f][h] = OP_BYTES + lds_off(wn * 64 + f * 16 + fr, 2 * fq + h);
    }

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 ra[LOADS], rb[LOADS];

  auto load_step = [&](int s) {
    const int k0 = s * BK8;
    const bool k_ok = k0 + ld_ch * 16 < d;    // d % 16 == 0: all or nothing
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
  auto fragment = [](const unsigned char* base, const int (&off)[2]) {
    const uint4 lo = *reinterpret_cast<const uint4*>(base + off[0]);
    const uint4 hi = *reinterpret_cast<const uint4*>(base + off[1]);
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                 (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };

  const int nsteps = (d + BK8 - 1) / BK8;
  load_step(0);
  store_step(0);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;
    if (more) load_step(s + 1);

    const unsigned char* base = lds + (s & 1) * BUF_BYTES;
    i32x8 bfr[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) bfr[f] = fragment(base, b_off[f]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const i32x8 af = fragment(base, a_off[i]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            TEXT_FIRST ? bfr[j] : af, TEXT_FIRST ? af : bfr[j], acc[i][j],
            0, 0,                                   // both operands e4m3
            0, MX_UNIT_SCALE, 0, MX_UNIT_SCALE);
    }

    if (more) store_step((s + 1) & 1);
    __syncthreads();
  }
}

// The main loop for MX operands (OCP MXFP8: e4m3 elements, one e8m0 scale per
// 32 consecutive k): zimg_q / ztxt_q as for pair_tile_dots_e4m3 with
// d % 32 == 0; zimg_e8 (b rows) and ztxt_e8 (n rows) hold one dword per row
// and 128-element K-step, byte kb of a row the e8m0 code of K-block kb, rows
// `lde` bytes apart (lde % 4 == 0, 4-byte aligned, at least 4·ceil(d / 128)).
// The contract of pair_tile_dots_e4m3 — acc layouts, zero-fill, 64-bit
// offsets, the closing barrier — except that acc holds the true dots
//   Σ_kb 2^(ea_kb − 127)·2^(eb_kb − 127)·Σ_{k in kb} a_k·b_k,
// the scaling done by the MFMA, and that `lds` holds MX_LDS_BYTES: the
// element slabs, staging thread map, lds_off and swizzle are the e4m3 loop's,
// and the 2 × 1 KiB above them take the scales.
//
// Fragments.  The instruction's k order is not the e4m3 loop's: lane l holds
// k = 16·(l >> 4) … +15 in its first four registers and k = 64 + 16·(l >> 4)
// … +15 in the other four, and scales the 32-element block of hardware k
// 32·kb … +31 by what lane group kb supplies (measured:
// tools/probe_mx_scale_map.hip sweeps every lane and byte of both scale
// operands; tools/probe_mx_rowscale.hip, with one scale per row, cannot
// tell).  With unit scales any pairing of equal k on both sides will do, which
// is what the e4m3 loop relies on; here a block must be 32 consecutive k of
// the row, so a lane reads chunks fq and 4 + fq of its fragment row instead
// of 2·fq and 2·fq + 1 — the bf16 loop's read pattern, conflict-free for the
// same reason.
//
// Scales.  Per step thread t < 128 loads image row m0 + t's dword, thread
// 128 + t text row n0 + t's (0x7F7F7F7F, 2⁰, for a row outside the block or a
// step past the scale row), together with its element chunks, and stores it
// with them: [128 image dwords][128 text dwords] per buffer, published by the
// barrier that publishes the elements.  The MFMA takes from lane l the scale
// of row l & 15, K-block l >> 4 — the lane's own fragment row and the byte
// fq = l >> 4 of that row's dword — so a lane reads the dword of each of its
// 4 + 4 fragment rows (16 consecutive dwords over a fragment's rows and the
// same address over its four K-blocks: conflict-free broadcasts) and one
// v_perm_b32 copies byte fq into all four bytes (the instruction reads the
// byte its op_sel names, byte 0 here).  8 ds_read_b32 and 8 v_perm_b32 per step against 40
// ds_read_b128 and 16 MFMAs; 8 more VGPRs than the e4m3 loop, the four text
// scales resident with their fragments, the image scales of the step too.
constexpr int MX_SCALE_BYTES = (BM + BN) * 4;              // one buffer: 1 KiB
constexpr int MX_LDS_BYTES = 2 * BUF_BYTES + 2 * MX_SCALE_BYTES;   // 66 KiB

// Operand element tag of the kernels that take MX operands: an e4m3 byte
// whose scale lives in a separate e8m0 array.
enum mx_e4m3 : unsigned char {};

// d a positive multiple of 32 on top of pair_dims_ok_e4m3, and scale rows of
// exactly one aligned dword per K-step.
inline bool pair_dims_ok_mx(const void* zimg_q, const void* zimg_e8,
                            const void* ztxt_q, const void* ztxt_e8, int b,
                            int n, int d, long long lde_img,
                            long long lde_txt) {
  if (!pair_dims_ok_e4m3(zimg_q, ztxt_q, b, n, d) || d % 32 != 0) return false;
  if (zimg_e8 == nullptr || ztxt_e8 == nullptr) return false;
  if (((uintptr_t)zimg_e8 | (uintptr_t)ztxt_e8) % 4 != 0) return false;
  const long long want = 4ll * ceil_div(d, BK8);
  return lde_img == want && lde_txt == want;
}

template <bool TEXT_FIRST>
__device__ __forceinline__ void pair_tile_dots_mx(
    const unsigned char* __restrict__ zimg_q,
    const unsigned char* __restrict__ zimg_e8,
    const unsigned char* __restrict__ ztxt_q,
    const unsigned char* __restrict__ ztxt_e8, int b, int n, int d, int lde,
    int m0, int n0, unsigned char* lds, f32x4 (&acc)[4][4]) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // Staging: thread t owns chunk t&7 of rows (t>>3) + 32·i, i = 0..3.
  const int ld_ch = tid & 7;
  const int ld_row = tid >> 3;
  const unsigned char* a_src[LOADS];
  const unsigned char* b_src[LOADS];
  bool a_ok[LOADS], b_ok[LOADS];
  int st_off[LOADS];
#pragma unroll
  for (int i = 0; i < LOADS; ++i) {
    const int row = ld_row + 32 * i;
    a_ok[i] = m0 + row < b;
    b_ok[i] = n0 + row < n;
    a_src[i] = zimg_q + (long long)(m0 + row) * d + ld_ch * 16;
    b_src[i] = ztxt_q + (long long)(n0 + row) * d + ld_ch * 16;
    st_off[i] = lds_off(row, ld_ch);
  }
  // ... and the scale dword of one row: image rows first.
  const bool sc_img = tid < BM;
  const int sc_row = sc_img ? m0 + tid : n0 + (tid - BM);
  const bool sc_ok = sc_row < (sc_img ? b : n);
  const unsigned char* sc_src =
      (sc_img ? zimg_e8 : ztxt_e8) + (long long)sc_row * lde;
  unsigned char* sc_lds = lds + 2 * BUF_BYTES;

  // Fragment reads: lane l takes row (l & 15), k = 16·(l >> 4) … +15 and
  // 64 + 16·(l >> 4) … +15 of the 128-deep MFMA step: chunks fq and 4 + fq.
  const int fr = lane & 15, fq = lane >> 4;
  int a_off[4][2], b_off[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      a_off[f][h] = lds_off(wm * 64 + f * 16 + fr, 4 * h + fq);
      b_off[f][h] = OP_BYTES + lds_off(wn * 64 + f * 16 + fr, 4 * h + fq);
    }
  const int sa_off = 4 * (wm * 64 + fr), sb_off = 4 * (BM + wn * 64 + fr);
  const unsigned fq_sel = 0x01010101u * (unsigned)fq;   // v_perm: byte fq × 4

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 ra[LOADS], rb[LOADS];
  unsigned rs;

  auto load_step = [&](int s) {
    const int k0 = s * BK8;
    const bool k_ok = k0 + ld_ch * 16 < d;    // d % 16 == 0: all or nothing
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      ra[i] = uint4{0u, 0u, 0u, 0u};
      rb[i] = uint4{0u, 0u, 0u, 0u};
      if (k_ok && a_ok[i])
        ra[i] = *reinterpret_cast<const uint4*>(a_src[i] + k0);
      if (k_ok && b_ok[i])
        rb[i] = *reinterpret_cast<const uint4*>(b_src[i] + k0);
    }
    rs = (unsigned)MX_UNIT_SCALE;
    if (sc_ok && 4 * s + 4 <= lde)
      rs = *reinterpret_cast<const unsigned*>(sc_src + 4 * s);
  };
  auto store_step = [&](int buf) {
    unsigned char* base = lds + buf * BUF_BYTES;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      *reinterpret_cast<uint4*>(base + st_off[i]) = ra[i];
      *reinterpret_cast<uint4*>(base + OP_BYTES + st_off[i]) = rb[i];
    }
    *reinterpret_cast<unsigned*>(sc_lds + buf * MX_SCALE_BYTES + 4 * tid) = rs;
  };
  auto fragment = [](const unsigned char* base, const int (&off)[2]) {
    const uint4 lo = *reinterpret_cast<const uint4*>(base + off[0]);
    const uint4 hi = *reinterpret_cast<const uint4*>(base + off[1]);
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                 (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };
  // Byte fq of fragment f's scale dword, in every byte.
  auto scale = [&](const unsigned char* sc, int off, int f) {
    const unsigned w = *reinterpret_cast<const unsigned*>(sc + off + 64 * f);
    return (int)__builtin_amdgcn_perm(0u, w, fq_sel);
  };

  const int nsteps = (d + BK8 - 1) / BK8;
  load_step(0);
  store_step(0);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;
    if (more) load_step(s + 1);

    const unsigned char* base = lds + (s & 1) * BUF_BYTES;
    const unsigned char* sc = sc_lds + (s & 1) * MX_SCALE_BYTES;
    i32x8 bfr[4];
    int sa[4], sb[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      bfr[f] = fragment(base, b_off[f]);
      sa[f] = scale(sc, sa_off, f);
      sb[f] = scale(sc, sb_off, f);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const i32x8 af = fragment(base, a_off[i]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            TEXT_FIRST ? bfr[j] : af, TEXT_FIRST ? af : bfr[j], acc[i][j],
            0, 0,                                   // both operands e4m3
            0, TEXT_FIRST ? sb[j] : sa[i], 0, TEXT_FIRST ? sa[i] : sb[j]);
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

// Sample ids (idlabel_kernels.hip, softmax_id_kernels.hip,
// rank_id_kernels.hip).  Stage the tile's
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

// The four row ids of fragment rows lrow0 … +3 (lrow0 % 4 == 0): what a lane
// owns in the !TEXT_FIRST layout.
__device__ __forceinline__ void load_row_ids(const long long* idl, int lrow0,
                                             long long (&rid)[4]) {
  const longlong2 r01 = *reinterpret_cast<const longlong2*>(idl + lrow0);
  const longlong2 r23 = *reinterpret_cast<const longlong2*>(idl + lrow0 + 2);
  rid[0] = r01.x; rid[1] = r01.y; rid[2] = r23.x; rid[3] = r23.y;
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

// The e4m3 slab pair (g and gᵀ, one byte per pair): two staging tiles of
// [128][G8_PITCH] bytes.  144 B = 36 dwords: the 4-byte writes of lanes (row
// or column index q = 0..15, dword a = 0..3) fall on banks 36·q + a, all 64
// distinct, and rows r and r + 8 start 32 banks apart, which is what
// store_g8_tile's 16-byte reads use.
constexpr int G8_PITCH = BN + 16;
constexpr int G8_TILE_BYTES = BM * G8_PITCH;  // 18 KiB each

// Four values of |v| ≤ 1 as OCP e4m3fn codes of 448·v (round to nearest
// even, saturating), v[0] in the low byte: what __hip_fp8_e4m3(448·v) gives
// for each, two at a time.  0 gives 0x00.
__device__ __forceinline__ unsigned pack_e4m3x4(f32x4 v) {
  float a[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    a[r] = __builtin_amdgcn_fmed3f(v[r] * 448.0f, 448.0f, -448.0f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], w, true);
  return (unsigned)w;
}

// 4×4 byte transpose inside a DPP quad (four adjacent lanes): lane c holds
// row c as one dword, byte k = column k; on return it holds column c, byte
// r = row r.  Two quad-permute moves (lane ^ 2, lane ^ 1) and two byte
// selects: 16-bit halves first, then bytes.  Every lane of the quad must be
// active.
__device__ __forceinline__ unsigned quad_transpose_bytes(unsigned x, int c) {
  unsigned y = (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xf, 0xf, true);
  x = __builtin_amdgcn_perm(y, x, (c & 2) ? 0x03020706u : 0x05040100u);
  y = (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xf, 0xf, true);
  return __builtin_amdgcn_perm(y, x, (c & 1) ? 0x03070105u : 0x06020400u);
}

// Write-out of one byte tile staged at `tile` ([128] rows at G8_PITCH bytes)
// into the (rows, cols) byte view `dst` of row stride ld, tile origin
// (r0, c0): 8 threads cover one 128-byte tile row, and a 16-lane group reads
// rows r and r + 8 (distinct banks).  A 16-byte store where the segment is
// whole and its address aligned, byte stores otherwise (ragged edge, odd row
// stride or offset); only elements of the view are touched.  g: rows are
// image rows; gᵀ: rows are text rows.  The caller's barrier orders the
// staging writes before this.
__device__ __forceinline__ void store_g8_tile(const unsigned char* tile,
                                              unsigned char* __restrict__ dst,
                                              long long ld, int r0, int c0,
                                              int rows, int cols) {
  const int tid = threadIdx.x;
  const int ch = tid & 7;
  const int lrow0 = ((tid >> 4) & 7) + 8 * ((tid >> 3) & 1) + 16 * (tid >> 7);
#pragma unroll
  for (int k = 0; k < BM / 32; ++k) {
    const int lrow = lrow0 + 32 * k;
    const int row = r0 + lrow, col = c0 + ch * 16;
    if (row >= rows || col >= cols) continue;
    const uint4 v =
        *reinterpret_cast<const uint4*>(tile + lrow * G8_PITCH + 16 * ch);
    unsigned char* p = dst + (long long)row * ld + col;
    if (col + 16 <= cols && ((uintptr_t)p & 15) == 0) {
      *reinterpret_cast<uint4*>(p) = v;
    } else {
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int x = 0; x < 16; ++x)
        if (col + x < cols) p[x] = (unsigned char)(w[x >> 2] >> (8 * (x & 3)));
    }
  }
}

}  // namespace
