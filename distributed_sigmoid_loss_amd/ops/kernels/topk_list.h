// What the two top-k kernels over the pair grid share (topk_kernels.hip,
// topk_id_kernels.hip; gfx950, MI355X): the running per-row list, the
// candidate buffer's layout, the fold of one tile's candidates into the list,
// the list capacities, and the kernel that merges the column spans' lists.
// Each including file adds its partials kernel (what makes an element a
// candidate) and its C entry point.  Everything sits in an anonymous
// namespace, so each translation unit gets its own copy.
//
// Order.  Higher score first, among equal scores the lower column first.  A
// partials kernel visits columns in ascending order over its span and the
// merge visits spans in ascending order, so a strict `>` at every comparison
// is the tie rule: of two equal scores the earlier column stays in front.
// The order is total and an element's fp32 score depends only on its own
// K-loop, so the result does not depend on how the columns are divided and is
// bitwise reproducible.  A predicate that only removes candidates changes
// none of this.

#pragma once

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

// Thread `tid` (< 128) folds the candidates of local row `tid` of the tile at
// column n0 into its list, in ascending column order.  mask[row][wave column]
// [lane group] holds bit 4·j + r for the element at local column
// 64·(wave column) + 16·j + 4·(lane group) + r; its score sits in
// cand[row][that column].
template <int KCAP>
__device__ __forceinline__ void fold_row_candidates(
    TopList<KCAP>& top, const unsigned short* mask, const float* cand, int tid,
    int n0) {
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

// The workspaces (n_splits, b, KCAP) → out (b, k).
template <int KCAP>
int launch_merge(hipStream_t stream, void* ws_s, void* ws_c, void* out_s,
                 void* out_c, int b, int k, int n_splits) {
  hipLaunchKernelGGL(pair_topk_merge_kernel<KCAP>,
                     dim3((unsigned)((b + NTHREADS - 1) / NTHREADS)),
                     dim3(NTHREADS), 0, stream, (const float*)ws_s,
                     (const int*)ws_c, (float*)out_s, (int*)out_c, b, k,
                     n_splits);
  return (int)hipGetLastError();
}

// What both C entries check beyond pair_dims_ok: workspaces and outputs given
// and 4-byte aligned, 1 ≤ n_splits ≤ tiles_n, a grid the block walk can index.
inline bool topk_args_ok(const void* ws_s, const void* ws_c, const void* out_s,
                         const void* out_c, int tiles_m, int tiles_n,
                         int n_splits) {
  if (ws_s == nullptr || ws_c == nullptr || out_s == nullptr ||
      out_c == nullptr)
    return false;
  if (((uintptr_t)ws_s | (uintptr_t)ws_c | (uintptr_t)out_s |
       (uintptr_t)out_c) % 4 != 0)
    return false;
  return n_splits >= 1 && n_splits <= tiles_n &&
         pair_grid_ok(tiles_m, n_splits);
}

}  // namespace
