// Fused top-k over the image×text pair grid for gfx950 (MI355X): the k best
// scoring columns of every row, without the grid ever reaching memory.
//
//   s_ij = <zimg_i, ztxt_j>                 zimg (b, d), ztxt (n, d) bf16
//   candidates of row i: the columns j in [0, n) with j != i + diag
//                        (diag = INT_MIN: nothing is excluded)
//   order: higher score first, among equal scores the lower column first
//   out[i][q] = the q-th candidate in that order as (score fp32, column int32),
//               (−inf, −1) once the candidates run out
//
// The order is total (columns are distinct) and an element's fp32 score
// depends only on its own K-loop, so the result does not depend on how the
// columns are divided among workgroups, is bitwise reproducible, and merges
// exactly over column chunks.  There is no atomic anywhere.
//
// Two kernels:
//
// - pair_topk_partials_kernel<KCAP>: a workgroup owns 128 image rows and split
//   `s` of `n_splits`, a contiguous span of 128-column tiles that it walks in
//   ascending order.  Every tile is pair_tile.h's 128×128 MFMA tile with the
//   text fragment first; the epilogue below folds it into a running sorted
//   list of KCAP (score, column) pairs per row.  After the last tile the
//   lists go to a workspace laid out (n_splits, b, KCAP).
// - pair_topk_merge_kernel<KCAP>: one thread per row folds the row's n_splits
//   workspace lists, in split order, into one list under the same total order
//   and writes its first k entries, the (−inf, −1) fill included.
//
// Tile.  pair_tile.h's, text fragment first: lane l owns image row (l & 15)
// and the four consecutive columns 4·(l >> 4) … +3 of each fragment.
//
// Epilogue: a per-row threshold.  thr[row] (LDS) is the score of the row's
// current KCAP-th entry, −inf while the list is not full.  Each lane compares
// its 64 elements with the thresholds of their rows.  An element that lies in
// the block, is not the excluded positive and scores strictly above the
// threshold is a candidate: the lane writes its score to the element's own
// slot of a [128][128] fp32 buffer (over the staging buffers, free after the
// k-loop's last barrier; its pitch is 129 so that the fold's reads fall on
// distinct banks) and sets the element's bit in a 16-bit mask
// that it leaves at mask[row][wave column][lane group].  Slots are fixed by
// position and only the owner writes one: nothing depends on arrival order.
// After a barrier thread `row` (the first 128 threads) walks the set bits of
// its row in ascending column order and inserts each candidate that still
// beats the list's last entry into the list, which it keeps in registers
// (a fully unrolled compare-swap chain), then publishes the new threshold.
// Columns are visited in ascending order over the whole span, so a strict
// `>` at every comparison is the tie rule: of two equal scores the earlier
// column stays in front.  Once the lists are warm almost nothing passes the
// threshold and a tile costs the comparisons, two barriers and one 16-byte
// mask read per row.  A zero-filled padding column scores 0 and would beat
// every negative score: it is never a candidate, nor is the positive.
//
// Placement.  A 1-D grid of tiles_m · n_splits workgroups; the block id is
// remapped so consecutive logical ids share an XCD, and logical id l owns
// tile-row l / n_splits and split l % n_splits: the splits of a tile-row sit
// on one XCD and share its image panel in L2.

#include "pair_tile.h"

namespace {

constexpr int MAX_K = 16;        // largest compiled list capacity

// Candidate buffer: [128][128] fp32 at a pitch of 129, so that the fold's
// reads (one thread per row, often the same column) fall on distinct banks.
// It overlays the staging buffers and needs 512 bytes more than they do.
constexpr int CAND_PITCH = BN + 1;
constexpr int LDS_BYTES = BM * CAND_PITCH * 4;

static_assert(LDS_BYTES >= 2 * BUF_BYTES, "staging buffers exceed the LDS");

// A row's running list, best first.  All indices are compile-time constants
// after unrolling, so the list stays in registers.
template <int KCAP>
struct TopList {
  float s[KCAP];
  int c[KCAP];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int q = 0; q < KCAP; ++q) {
      s[q] = -__builtin_inff();
      c[q] = -1;
    }
  }

  // `col` is larger than every column already in the list: the new entry
  // belongs behind every entry that scores at least as high.
  __device__ __forceinline__ void insert(float v, int col) {
    if (!(v > s[KCAP - 1])) return;
    s[KCAP - 1] = v;
    c[KCAP - 1] = col;
#pragma unroll
    for (int q = KCAP - 2; q >= 0; --q) {
      const bool up = s[q + 1] > s[q];
      const float hs = up ? s[q + 1] : s[q], ls = up ? s[q] : s[q + 1];
      const int hc = up ? c[q + 1] : c[q], lc = up ? c[q] : c[q + 1];
      s[q] = hs; s[q + 1] = ls;
      c[q] = hc; c[q + 1] = lc;
    }
  }
};

__device__ __forceinline__ unsigned nib(unsigned x, int sh) {
  return (x >> sh) & 0xfu;
}

template <int KCAP>
__launch_bounds__(NTHREADS) __global__ void pair_topk_partials_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    float* __restrict__ ws_s, int* __restrict__ ws_c, int b, int n, int d,
    int diag, int tiles_m, int tiles_n, int n_splits) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
  __shared__ __attribute__((aligned(16))) unsigned short mask[BM * 8];
  __shared__ float thr[BM];

  // XCD-contiguous (bijective) remap; splits of a tile-row are neighbours.
  const int lid = xcd_logical_id(tiles_m * n_splits);
  const int tm = lid / n_splits, split = lid - tm * n_splits;
  const int m0 = tm * BM;
  // Split s owns column tiles [s·T/S, (s+1)·T/S): never empty as S ≤ T.
  const int t_begin = (int)((long long)split * tiles_n / n_splits);
  const int t_end = (int)((long long)(split + 1) * tiles_n / n_splits);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  float* cand = reinterpret_cast<float*>(lds);

  // Per image row of this lane: inside the block?  Column of its positive,
  // −1 when there is none in the block.
  bool row_ok[4];
  int pc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = m0 + wm * 64 + i * 16 + fr;
    row_ok[i] = row < b;
    pc[i] = positive_col(row, diag, n);
  }

  TopList<KCAP> top;             // used by threads 0..127: row m0 + tid
  top.clear();
  if (tid < BM) thr[tid] = -__builtin_inff();
  // The first tile's barriers order this store before the first read.

  for (int tn = t_begin; tn < t_end; ++tn) {
    const int n0 = tn * BN;
    f32x4 acc[4][4];
    pair_tile_dots<true>(zimg, ztxt, b, n, d, m0, n0, lds, acc);

    // Candidates: score to the element's slot, bit 4·j + r to the lane mask.
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lrow = wm * 64 + i * 16 + fr;
      const float t = thr[lrow];
      // Relative to this lane's first column, c0: the element (j, r) is
      // column c0 + 16·j + r, so every comparison is against a constant.
      const int c0 = n0 + wn * 64 + fq * 4;
      const int n_rel = row_ok[i] ? n - c0 : 0, pc_rel = pc[i] - c0;
      float* slot = cand + lrow * CAND_PITCH + wn * 64 + fq * 4;
      unsigned mk = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = acc[i][j][r];
          if (16 * j + r < n_rel && 16 * j + r != pc_rel && s > t) {
            slot[16 * j + r] = s;
            mk |= 1u << (4 * j + r);
          }
        }
      mask[lrow * 8 + wn * 4 + fq] = (unsigned short)mk;
    }
    __syncthreads();

    // Fold: thread `row` takes its candidates in ascending column order.
    if (tid < BM) {
      const uint4 hv = *reinterpret_cast<const uint4*>(mask + tid * 8);
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        // lo: lane groups 0 (low half) and 1, hi: groups 2 and 3.
        const unsigned lo = w ? hv.z : hv.x, hi = w ? hv.w : hv.y;
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
          // Bit jj·16 + fq·4 + r of m: fragment 2·jp + jj of wave column w.
          unsigned m = 0;
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int sh = 8 * jp + 4 * jj;
            m |= (nib(lo, sh) | (nib(lo, 16 + sh) << 4) | (nib(hi, sh) << 8) |
                  (nib(hi, 16 + sh) << 12)) << (16 * jj);
          }
          const int base = w * 64 + jp * 32;
          while (m != 0) {
            const int lcol = base + __builtin_ctz(m);
            m &= m - 1;
            top.insert(cand[tid * CAND_PITCH + lcol], n0 + lcol);
          }
        }
      }
      thr[tid] = top.s[KCAP - 1];
    }
    // Orders the fold's reads before the next tile's staging stores, and the
    // new thresholds before their readers.
    __syncthreads();
  }

  if (tid < BM && m0 + tid < b) {
    const long long o = ((long long)split * b + (m0 + tid)) * KCAP;
#pragma unroll
    for (int q = 0; q < KCAP; ++q) {
      ws_s[o + q] = top.s[q];
      ws_c[o + q] = top.c[q];
    }
  }
}

// One thread per row: fold the row's n_splits lists, split 0 first, into one
// list with the partials kernel's insert.  Its precondition holds: spans are
// ascending column ranges and each list is sorted, so every entry arrives
// after all entries with a lower column that score the same.
template <int KCAP>
__launch_bounds__(NTHREADS) __global__ void pair_topk_merge_kernel(
    const float* __restrict__ ws_s, const int* __restrict__ ws_c,
    float* __restrict__ out_s, int* __restrict__ out_c, int b, int k,
    int n_splits) {
  const long long row = (long long)blockIdx.x * NTHREADS + threadIdx.x;
  if (row >= b) return;
  TopList<KCAP> top;
  top.clear();
  for (int sp = 0; sp < n_splits; ++sp) {
    const long long o = ((long long)sp * b + row) * KCAP;
    float s[KCAP];
    int c[KCAP];
#pragma unroll
    for (int e = 0; e < KCAP; ++e) {
      s[e] = ws_s[o + e];
      c[e] = ws_c[o + e];
    }
#pragma unroll
    for (int e = 0; e < KCAP; ++e)
      if (c[e] >= 0) top.insert(s[e], c[e]);   // c < 0: fill
  }
#pragma unroll
  for (int q = 0; q < KCAP; ++q)
    if (q < k) {
      out_s[row * k + q] = top.s[q];
      out_c[row * k + q] = top.c[q];
    }
}

int capacity_for(int k) {
  if (k < 1 || k > MAX_K) return 0;
  return k <= 1 ? 1 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
}

template <int KCAP>
int launch(hipStream_t stream, const void* zimg, const void* ztxt, void* ws_s,
           void* ws_c, void* out_s, void* out_c, int b, int n, int d, int diag,
           int k, int tiles_m, int tiles_n, int n_splits) {
  hipLaunchKernelGGL(pair_topk_partials_kernel<KCAP>,
                     dim3(tiles_m * n_splits), dim3(NTHREADS), 0, stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt, (float*)ws_s,
                     (int*)ws_c, b, n, d, diag, tiles_m, tiles_n, n_splits);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  hipLaunchKernelGGL(pair_topk_merge_kernel<KCAP>,
                     dim3((unsigned)((b + NTHREADS - 1) / NTHREADS)),
                     dim3(NTHREADS), 0, stream, (const float*)ws_s,
                     (const int*)ws_c, (float*)out_s, (int*)out_c, b, k,
                     n_splits);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// Largest k the kernel serves.
int pair_topk_max_k() { return MAX_K; }

// Edge of the square tile: n_splits is at most ceil(n / tile).
int pair_topk_tile_dim() { return BN; }

// List capacity that serves k (0: unsupported k).  The workspaces hold
// n_splits · b · capacity entries each.
int pair_topk_capacity(int k) { return capacity_for(k); }

// out_s / out_c (b, k): the k best candidates of every row of the (b, n)
// block of zimg (b, d) × ztxt (n, d), bf16 row-major contiguous, skipping
// j == i + diag (INT_MIN: nothing).  ws_s (fp32) and ws_c (int32) hold
// n_splits · b · pair_topk_capacity(k) entries.  Returns non-zero, launching
// nothing, on anything unsupported: null pointers, k outside [1, max],
// n_splits outside [1, ceil(n / tile)], d not a positive multiple of 8,
// misaligned pointers.
int pair_topk_bf16(uintptr_t stream, const void* zimg, const void* ztxt,
                   void* ws_s, void* ws_c, void* out_s, void* out_c, int b,
                   int n, int d, int diag, int k, int n_splits) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d) || ws_s == nullptr ||
      ws_c == nullptr || out_s == nullptr || out_c == nullptr)
    return (int)hipErrorInvalidValue;
  const int kcap = capacity_for(k);
  if (kcap == 0) return (int)hipErrorInvalidValue;
  if (((uintptr_t)ws_s | (uintptr_t)ws_c | (uintptr_t)out_s |
       (uintptr_t)out_c) % 4 != 0)
    return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (n_splits < 1 || n_splits > tiles_n ||
      !pair_grid_ok(tiles_m, n_splits))
    return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
#define TOPK_LAUNCH(KCAP)                                                     \
  launch<KCAP>(st, zimg, ztxt, ws_s, ws_c, out_s, out_c, b, n, d, diag, k,    \
               tiles_m, tiles_n, n_splits)
  switch (kcap) {
    case 1: return TOPK_LAUNCH(1);
    case 4: return TOPK_LAUNCH(4);
    case 8: return TOPK_LAUNCH(8);
    default: return TOPK_LAUNCH(16);
  }
#undef TOPK_LAUNCH
}

}  // extern "C"
