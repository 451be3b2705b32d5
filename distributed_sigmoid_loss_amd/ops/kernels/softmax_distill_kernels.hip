// Softmax distillation loss (the KL form) for gfx950 (MI355X): the student's
// row and column softmax over the image×text grid pulled towards a teacher
// dual encoder's, mixed with the hard InfoNCE label.  Two (b, n) grids of dot
// products — the teacher's and the student's — are evaluated tile by tile in
// each kernel, and neither is ever written to memory.
//
//   z_ij = t·<zimg_i, ztxt_j>,   t   = exp(t')        (student)
//   v_ij = t_T·<timg_i, ttxt_j>, t_T = exp(t'_T)      (teacher)
//   LS^r_i = log Σ_j exp z_ij    LT^r_i = log Σ_j exp v_ij     (columns alike)
//   x^r_i  = Σ_j exp(v_ij − LT^r_i)·(v_ij − z_ij)
//   KL(P^r_i ‖ softmax z_i) = LS^r_i − LT^r_i + x^r_i
//   g_ij = rw_i·exp(z_ij − LS^r_i) + cw_j·exp(z_ij − LS^c_j) − T_ij
//   T_ij = rtw_i·exp(v_ij − LT^r_i) + ctw_j·exp(v_ij − LT^c_j)
//          + [j == i + diag]·(rhw_i + chw_j)
//
// Three kernels:
//
// - softmax_distill_stats_kernel: per 128×128 tile, one 32-byte record per row
//   over the tile's columns and per column over the tile's rows,
//     (max z, Σ exp(z − max z), max v, Σ exp(v − max v),
//      Σ exp(v − max v)·(v − z)),
//   in workspaces laid out (tiles_n, b) and (tiles_m, n).  The weighted sum
//   rides on the teacher's own running max, so it folds across waves, tiles,
//   column chunks and ranks by the factor that folds the teacher's Σ exp.
// - softmax_distill_finish_kernel: one thread per row / column folds its
//   records in tile order into lse_s, lse_t and the normalised x.
// - softmax_distill_g_kernel: the epilogue evaluates g, stages the bf16 tile
//   in LDS and writes it as coalesced 16-byte row segments into a (b, n) view
//   of row stride ldg, and leaves one fp32 partial Σ g_ij·s_ij (s = z / t) per
//   tile.
//
// There is no atomic and no counter anywhere: every reduction has a fixed
// order (xor shuffles, the two or four waves in wave order, tiles in tile
// order), so all results are bitwise reproducible.
//
// Two K loops, one LDS (the pattern of distill_kernels.hip).  pair_tile.h's
// main loop runs twice in the same 64 KiB of operand slabs — it ends on a
// barrier, so the second run may overwrite what the first one staged — first
// over the teacher pair (timg, ttxt, d_T), then over the student pair (zimg,
// ztxt, d), each with its own zero-filled K tail.  A lane holds 128
// accumulators, 64 of them live in the MFMA at any time: two workgroups per
// CU (__launch_bounds__(256, 2), 256 VGPRs + AGPRs per lane).
//
// Stats kernel.  The 64 raw teacher dots stay in fp32 registers across the
// student loop.  The epilogue replaces everything outside the block by −inf
// in both grids (a zero-filled padding column scores 0, which would dominate
// a row of negative logits) and walks the fragments column by column: a
// fragment's four columns are complete in this wave once its four rows are
// through, so they are reduced right away, and only the rows' running maxima
// are carried to the row pass that follows.  v − z of a masked element is
// taken as 0, never as inf − inf.
//
// g kernel.  After the teacher loop its 64 accumulators become, in place,
// the target term T.  The teacher-side column vectors (LT^c, ctw, chw) are
// read fragment column by fragment column and, like the row ones, are dead
// before the student loop: ten per-column vectors do not fit next to 128
// accumulators.  T stays fp32: g is a difference of probabilities, and a
// bf16 T would put 2⁻⁹ into it.  A skipped side adds no term at all; padding
// is set to exactly 0.
//
// exp / log are the bare v_exp_f32 / v_log_f32 (base 2) with the log2 e
// factors folded into the scale of the argument and of the result.

#include "pair_tile.h"

#include <type_traits>

namespace {

// One row's or column's statistics over a tile (or half a tile, in LDS, where
// mz and mv are maxima of raw dots; in memory they are in units of z and v).
struct __attribute__((aligned(16))) Record {
  float mz;    // max z
  float sz;    // Σ exp(z − mz)
  float mv;    // max v
  float sv;    // Σ exp(v − mv)
  float x;     // Σ exp(v − mv)·(v − z)
  float pad[3];
};
static_assert(sizeof(Record) == 32, "two 16-byte stores per record");

// Stats kernel: part_row[wn][128], part_col[wm][128].
static_assert(2 * (BM + BN) * (int)sizeof(Record) <= 2 * BUF_BYTES,
              "epilogue staging exceeds LDS");
// g kernel: 4 waves × 1 partial above the g staging.
static_assert(G_STAGE_BYTES + 16 <= 2 * BUF_BYTES, "g staging exceeds LDS");

__device__ __forceinline__ void put_record(Record* dst, float mz, float sz,
                                           float mv, float sv, float x) {
  float4* p = reinterpret_cast<float4*>(dst);
  p[0] = float4{mz, sz, mv, sv};
  p[1] = float4{x, 0.f, 0.f, 0.f};
}

// The teacher's K loop by operand element TOP: __bf16, or mx_e4m3 with the
// block scales in timg_e8 / ttxt_e8, rows lde bytes apart (the true dots of
// the dequantised values; `lds` then holds MX_LDS_BYTES).
template <typename TOP>
__device__ __forceinline__ void teacher_dots(
    const TOP* __restrict__ timg, const TOP* __restrict__ ttxt,
    const unsigned char* __restrict__ timg_e8,
    const unsigned char* __restrict__ ttxt_e8, int b, int n, int d_t, int lde,
    int m0, int n0, unsigned char* lds, f32x4 (&acc)[4][4]) {
  if constexpr (std::is_same<TOP, mx_e4m3>::value)
    pair_tile_dots_mx<true>((const unsigned char*)timg, timg_e8,
                            (const unsigned char*)ttxt, ttxt_e8, b, n, d_t,
                            lde, m0, n0, lds, acc);
  else
    pair_tile_dots<true>(timg, ttxt, b, n, d_t, m0, n0, lds, acc);
}

template <typename TOP>
constexpr int teacher_lds_bytes() {
  return std::is_same<TOP, mx_e4m3>::value ? MX_LDS_BYTES : 2 * BUF_BYTES;
}

template <typename TOP = __bf16>
__launch_bounds__(NTHREADS, 2) __global__ void softmax_distill_stats_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const TOP* __restrict__ timg,
    const TOP* __restrict__ ttxt, const float* __restrict__ tprime_t,
    Record* __restrict__ row_ws, Record* __restrict__ col_ws, int b, int n,
    int d, int d_t, int tiles_m, int tiles_n,
    const unsigned char* __restrict__ timg_e8,
    const unsigned char* __restrict__ ttxt_e8, int lde) {
  __shared__ __attribute__((aligned(16))) unsigned char
      lds[teacher_lds_bytes<TOP>()];
  const TilePos tp = tile_of_block(tiles_m, tiles_n);
  const int m0 = tp.tm * BM, n0 = tp.tn * BN;

  // Teacher first; its raw dots wait in registers.
  f32x4 tv[4][4];
  teacher_dots(timg, ttxt, timg_e8, ttxt_e8, b, n, d_t, lde, m0, n0, lds, tv);
  f32x4 acc[4][4];
  pair_tile_dots<true>(zimg, ztxt, b, n, d, m0, n0, lds, acc);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const float inf = __builtin_inff();
  const float t = expf(tprime[0]), tt = expf(tprime_t[0]);
  const float sc2 = t * LOG2E, tc2 = tt * LOG2E;
  const bool rows_on = row_ws != nullptr;
  const bool cols_on = col_ws != nullptr;

  bool row_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) row_ok[i] = m0 + wm * 64 + i * 16 + fr < b;

  Record* part_row = reinterpret_cast<Record*>(lds);
  Record* part_col = part_row + 2 * BM;

  // v − z of an element, 0 outside the block.
  auto diff = [&](float s, float u) {
    return u == -inf ? 0.f : __builtin_fmaf(u, tt, -(s * t));
  };

  // Fragment column by fragment column: mask, reduce the four columns, carry
  // the rows' maxima.
  float rmz[4], rmv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rmz[i] = rmv[i] = -inf;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int lcol0 = wn * 64 + j * 16 + fq * 4;
    bool col_ok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) col_ok[r] = n0 + lcol0 + r < n;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // Whole fragments at a time: element writes into a live accumulator
      // make the compiler copy it.
      const f32x4 a = acc[i][j], u = tv[i][j];
      f32x4 am, um;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = row_ok[i] && col_ok[r];
        am[r] = ok ? a[r] : -inf;
        um[r] = ok ? u[r] : -inf;
      }
      acc[i][j] = am;
      tv[i][j] = um;
      rmz[i] = fmaxf(rmz[i], fmaxf(fmaxf(am[0], am[1]), fmaxf(am[2], am[3])));
      rmv[i] = fmaxf(rmv[i], fmaxf(fmaxf(um[0], um[1]), fmaxf(um[2], um[3])));
    }
    if (cols_on) {
      // A column lives in the 16 lanes that share fq (lane bits 0-3).
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mz = fmaxf(fmaxf(acc[0][j][r], acc[1][j][r]),
                         fmaxf(acc[2][j][r], acc[3][j][r]));
        float mv = fmaxf(fmaxf(tv[0][j][r], tv[1][j][r]),
                         fmaxf(tv[2][j][r], tv[3][j][r]));
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) {
          mz = fmaxf(mz, __shfl_xor(mz, x, 64));
          mv = fmaxf(mv, __shfl_xor(mv, x, 64));
        }
        const float mzs = safe_max(mz), mvs = safe_max(mv);
        float sz = 0.f, sv = 0.f, xs = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = acc[i][j][r], u = tv[i][j][r];
          sz += __builtin_amdgcn_exp2f((s - mzs) * sc2);
          const float ev = __builtin_amdgcn_exp2f((u - mvs) * tc2);
          sv += ev;
          xs = __builtin_fmaf(ev, diff(s, u), xs);
        }
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) {
          sz += __shfl_xor(sz, x, 64);
          sv += __shfl_xor(sv, x, 64);
          xs += __shfl_xor(xs, x, 64);
        }
        if (fr == 0)
          put_record(part_col + wm * BN + lcol0 + r, mz, sz, mv, sv, xs);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  if (rows_on) {
    // A row lives in the 4 lanes that share fr (lane bits 4-5).
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float mz = rmz[i], mv = rmv[i];
      mz = fmaxf(mz, __shfl_xor(mz, 16, 64));
      mv = fmaxf(mv, __shfl_xor(mv, 16, 64));
      mz = fmaxf(mz, __shfl_xor(mz, 32, 64));
      mv = fmaxf(mv, __shfl_xor(mv, 32, 64));
      const float mzs = safe_max(mz), mvs = safe_max(mv);
      float sz = 0.f, sv = 0.f, xs = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = acc[i][j][r], u = tv[i][j][r];
          sz += __builtin_amdgcn_exp2f((s - mzs) * sc2);
          const float ev = __builtin_amdgcn_exp2f((u - mvs) * tc2);
          sv += ev;
          xs = __builtin_fmaf(ev, diff(s, u), xs);
        }
#pragma unroll
      for (int x = 16; x <= 32; x <<= 1) {
        sz += __shfl_xor(sz, x, 64);
        sv += __shfl_xor(sv, x, 64);
        xs += __shfl_xor(xs, x, 64);
      }
      if (fq == 0)
        put_record(part_row + wn * BM + wm * 64 + i * 16 + fr, mz, sz, mv, sv,
                   xs);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();

  // Fold the two waves of each row / column (wave 0 first) and store.
  const bool row_half = tid < BM;
  const int e = row_half ? tid : tid - BM;
  if (row_half ? !rows_on : !cols_on) return;
  const Record* part = row_half ? part_row : part_col;
  const Record p0 = part[e], p1 = part[BM + e];
  const float mz = fmaxf(p0.mz, p1.mz), mv = fmaxf(p0.mv, p1.mv);
  const float mzs = safe_max(mz), mvs = safe_max(mv);
  const float sz = p0.sz * __builtin_amdgcn_exp2f((p0.mz - mzs) * sc2) +
                   p1.sz * __builtin_amdgcn_exp2f((p1.mz - mzs) * sc2);
  const float w0 = __builtin_amdgcn_exp2f((p0.mv - mvs) * tc2);
  const float w1 = __builtin_amdgcn_exp2f((p1.mv - mvs) * tc2);
  const float sv = p0.sv * w0 + p1.sv * w1;
  const float xs = p0.x * w0 + p1.x * w1;
  if (row_half) {
    if (m0 + e < b)
      put_record(row_ws + (long long)tp.tn * b + (m0 + e), mz * t, sz,
                 mv * tt, sv, xs);
  } else {
    if (n0 + e < n)
      put_record(col_ws + (long long)tp.tm * n + (n0 + e), mz * t, sz,
                 mv * tt, sv, xs);
  }
}

// The three results of one side.
struct StatsOut { float *lse_s, *lse_t, *x; };

// One thread per row (ids 0 … b−1, when the row side is given) or column (the
// ids after them): fold `tiles` records, tile 0 first.
__launch_bounds__(NTHREADS) __global__ void softmax_distill_finish_kernel(
    const Record* __restrict__ row_ws, const Record* __restrict__ col_ws,
    StatsOut row_out, StatsOut col_out, int b, int n, int tiles_m,
    int tiles_n) {
  const long long id = (long long)blockIdx.x * NTHREADS + threadIdx.x;
  const long long nrows = row_ws != nullptr ? b : 0;
  const long long ncols = col_ws != nullptr ? n : 0;
  const Record* ws;
  StatsOut out;
  long long len, e;
  int tiles;
  if (id < nrows) {
    ws = row_ws; out = row_out; len = b; e = id; tiles = tiles_n;
  } else if (id - nrows < ncols) {
    ws = col_ws; out = col_out; len = n; e = id - nrows; tiles = tiles_m;
  } else {
    return;
  }
  float mz = -__builtin_inff(), mv = -__builtin_inff();
  for (int k = 0; k < tiles; ++k) {
    const float4 p = *reinterpret_cast<const float4*>(ws + k * len + e);
    mz = fmaxf(mz, p.x);
    mv = fmaxf(mv, p.z);
  }
  const float mzs = safe_max(mz), mvs = safe_max(mv);
  float sz = 0.f, sv = 0.f, xs = 0.f;
  for (int k = 0; k < tiles; ++k) {
    const Record p = ws[k * len + e];
    sz += p.sz * __builtin_amdgcn_exp2f((p.mz - mzs) * LOG2E);
    const float w = __builtin_amdgcn_exp2f((p.mv - mvs) * LOG2E);
    sv += p.sv * w;
    xs += p.x * w;
  }
  out.lse_s[e] = mz + LN2 * __builtin_amdgcn_logf(sz);
  out.lse_t[e] = mv + LN2 * __builtin_amdgcn_logf(sv);
  out.x[e] = xs / sv;
}

// What the g kernel reads of one side: the student's and the teacher's LSE,
// the weight of the student's softmax (w = tw + hw), of the teacher's (tw) and
// of the hard positive (hw).  All five or none.
struct SideVecs { const float *lse_s, *lse_t, *w, *tw, *hw; };

template <typename TOP = __bf16>
__launch_bounds__(NTHREADS, 2) __global__ void softmax_distill_g_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const TOP* __restrict__ timg,
    const TOP* __restrict__ ttxt, const float* __restrict__ tprime_t,
    SideVecs rv, SideVecs cv, __bf16* __restrict__ g,
    float* __restrict__ gs_ws, int b, int n, int d, int d_t, long long ldg,
    int diag, int tiles_m, int tiles_n,
    const unsigned char* __restrict__ timg_e8,
    const unsigned char* __restrict__ ttxt_e8, int lde) {
  __shared__ __attribute__((aligned(16))) unsigned char
      lds[teacher_lds_bytes<TOP>()];
  const TilePos tp = tile_of_block(tiles_m, tiles_n);
  const int m0 = tp.tm * BM, n0 = tp.tn * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const bool rows_on = rv.lse_s != nullptr;
  const bool cols_on = cv.lse_s != nullptr;

  // Teacher: dots, then the target term in place.
  f32x4 tg[4][4];
  teacher_dots(timg, ttxt, timg_e8, ttxt_e8, b, n, d_t, lde, m0, n0, lds, tg);
  {
    const float tc2 = expf(tprime_t[0]) * LOG2E;
    float rl2[4], rtw[4], rhw[4];
    int pc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned row = m0 + wm * 64 + i * 16 + fr;
      const bool on = rows_on && row < (unsigned)b;
      rl2[i] = on ? -rv.lse_t[row] * LOG2E : 0.f;
      rtw[i] = on ? rv.tw[row] : 0.f;
      rhw[i] = on ? rv.hw[row] : 0.f;
      pc[i] = positive_col((int)row, diag, n);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned col0 = n0 + wn * 64 + j * 16 + fq * 4;
      float cl2[4], ctw[4], chw[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = cols_on && col0 + r < (unsigned)n;
        cl2[r] = on ? -cv.lse_t[col0 + r] * LOG2E : 0.f;
        ctw[r] = on ? cv.tw[col0 + r] : 0.f;
        chw[r] = on ? cv.hw[col0 + r] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 uv = tg[i][j];
        f32x4 out;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float u = uv[r];
          // A skipped side adds no term at all (never 0 · exp(…)).
          float tgt = 0.f;
          if (rows_on)
            tgt += rtw[i] * __builtin_amdgcn_exp2f(
                       __builtin_fmaf(u, tc2, rl2[i]));
          if (cols_on)
            tgt += ctw[r] * __builtin_amdgcn_exp2f(
                       __builtin_fmaf(u, tc2, cl2[r]));
          if ((int)(col0 + r) == pc[i]) tgt += rhw[i] + chw[r];
          out[r] = tgt;
        }
        // Pinned here: T's only reader is the epilogue, and left alone the
        // compiler sinks this conversion past the student loop and carries
        // the teacher's vectors through it instead.
        asm volatile("" : "+v"(out));
        tg[i][j] = out;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // Student: the same LDS, a second accumulator set.
  f32x4 acc[4][4];
  pair_tile_dots<true>(zimg, ztxt, b, n, d, m0, n0, lds, acc);
  // The student's vectors are read after the loop, not carried through it.
  asm volatile("" ::: "memory");

  const float sc2 = expf(tprime[0]) * LOG2E;
  float rl2[4], rw[4];
  bool row_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned row = m0 + wm * 64 + i * 16 + fr;
    row_ok[i] = row < (unsigned)b;
    const bool on = rows_on && row_ok[i];
    rl2[i] = on ? -rv.lse_s[row] * LOG2E : 0.f;
    rw[i] = on ? rv.w[row] : 0.f;
  }

  float s_gs = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int lcol0 = wn * 64 + j * 16 + fq * 4;
    const unsigned col0 = n0 + lcol0;
    float cl2[4], cw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = cols_on && col0 + r < (unsigned)n;
      cl2[r] = on ? -cv.lse_s[col0 + r] * LOG2E : 0.f;
      cw[r] = on ? cv.w[col0 + r] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x4 out;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[i][j][r];
        float gv = 0.f;
        if (rows_on)
          gv += rw[i] * __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, rl2[i]));
        if (cols_on)
          gv += cw[r] * __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, cl2[r]));
        gv -= tg[i][j][r];
        if (!(row_ok[i] && col0 + r < (unsigned)n)) gv = 0.f;
        s_gs = __builtin_fmaf(gv, s, s_gs);
        out[r] = (__bf16)gv;
      }
      *reinterpret_cast<bf16x4*>(lds + (wm * 64 + i * 16 + fr) * G_PITCH
                                 + 2 * lcol0) = out;
    }
    __builtin_amdgcn_sched_barrier(0);
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

// The teacher pair as an entry received it: bf16 rows (img, txt; mx false),
// or MXFP8 — e4m3 rows plus their e8m0 scale rows, lde bytes apart.
struct Teacher {
  const void *img, *txt, *img_e8, *txt_e8;
  long long lde;
  bool mx;
};

// What all entries check alike: the two pairs, the two temperatures and the
// grid size.
bool dims_ok(const void* zimg, const void* ztxt, const void* tprime,
             const Teacher& te, const void* tprime_t, int b, int n, int d,
             int d_t) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d)) return false;
  if (te.mx ? !pair_dims_ok_mx(te.img, te.img_e8, te.txt, te.txt_e8, b, n, d_t,
                               te.lde, te.lde)
            : !pair_dims_ok(te.img, te.txt, b, n, d_t))
    return false;
  if (tprime == nullptr || tprime_t == nullptr ||
      ((uintptr_t)tprime | (uintptr_t)tprime_t) % 4 != 0)
    return false;
  return pair_grid_ok(ceil_div(b, BM), ceil_div(n, BN));
}

// All of a side's pointers or none of them, each 4-byte aligned: 1 all,
// 0 none, −1 neither.
int side_state(const void* const* p, int count) {
  int given = 0;
  uintptr_t bits = 0;
  for (int k = 0; k < count; ++k) {
    given += p[k] != nullptr;
    bits |= (uintptr_t)p[k];
  }
  if ((given != 0 && given != count) || bits % 4 != 0) return -1;
  return given != 0;
}

template <typename TOP>
void launch_stats(hipStream_t stream, const void* zimg, const void* ztxt,
                  const void* tprime, const Teacher& te, const void* tprime_t,
                  void* row_ws, void* col_ws, int b, int n, int d, int d_t,
                  int tiles_m, int tiles_n) {
  hipLaunchKernelGGL(softmax_distill_stats_kernel<TOP>,
                     dim3(tiles_m * tiles_n), dim3(NTHREADS), 0, stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt,
                     (const float*)tprime, (const TOP*)te.img,
                     (const TOP*)te.txt, (const float*)tprime_t,
                     (Record*)row_ws, (Record*)col_ws, b, n, d, d_t, tiles_m,
                     tiles_n, (const unsigned char*)te.img_e8,
                     (const unsigned char*)te.txt_e8, (int)te.lde);
}

int stats_entry(uintptr_t stream, const void* zimg, const void* ztxt,
                const void* tprime, const Teacher& te, const void* tprime_t,
                void* row_ws, void* col_ws, void* row_lse_s, void* row_lse_t,
                void* row_x, void* col_lse_s, void* col_lse_t, void* col_x,
                int b, int n, int d, int d_t) {
  if (!dims_ok(zimg, ztxt, tprime, te, tprime_t, b, n, d, d_t))
    return (int)hipErrorInvalidValue;
  const void* const rp[4] = {row_ws, row_lse_s, row_lse_t, row_x};
  const void* const cp[4] = {col_ws, col_lse_s, col_lse_t, col_x};
  const int rows = side_state(rp, 4), cols = side_state(cp, 4);
  if (rows < 0 || cols < 0 ||
      ((uintptr_t)row_ws | (uintptr_t)col_ws) % 16 != 0)
    return (int)hipErrorInvalidValue;
  if (!rows && !cols) return 0;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (te.mx)
    launch_stats<mx_e4m3>((hipStream_t)stream, zimg, ztxt, tprime, te,
                          tprime_t, row_ws, col_ws, b, n, d, d_t, tiles_m,
                          tiles_n);
  else
    launch_stats<__bf16>((hipStream_t)stream, zimg, ztxt, tprime, te,
                         tprime_t, row_ws, col_ws, b, n, d, d_t, tiles_m,
                         tiles_n);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  const long long ids = (rows ? (long long)b : 0) + (cols ? (long long)n : 0);
  hipLaunchKernelGGL(softmax_distill_finish_kernel,
                     dim3((unsigned)((ids + NTHREADS - 1) / NTHREADS)),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const Record*)row_ws, (const Record*)col_ws,
                     StatsOut{(float*)row_lse_s, (float*)row_lse_t,
                              (float*)row_x},
                     StatsOut{(float*)col_lse_s, (float*)col_lse_t,
                              (float*)col_x},
                     b, n, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

template <typename TOP>
void launch_g(hipStream_t stream, const void* zimg, const void* ztxt,
              const void* tprime, const Teacher& te, const void* tprime_t,
              SideVecs rv, SideVecs cv, void* g, void* gs_ws, int b, int n,
              int d, int d_t, long long ldg, int diag, int tiles_m,
              int tiles_n) {
  hipLaunchKernelGGL(softmax_distill_g_kernel<TOP>, dim3(tiles_m * tiles_n),
                     dim3(NTHREADS), 0, stream, (const __bf16*)zimg,
                     (const __bf16*)ztxt, (const float*)tprime,
                     (const TOP*)te.img, (const TOP*)te.txt,
                     (const float*)tprime_t, rv, cv, (__bf16*)g,
                     (float*)gs_ws, b, n, d, d_t, ldg, diag, tiles_m, tiles_n,
                     (const unsigned char*)te.img_e8,
                     (const unsigned char*)te.txt_e8, (int)te.lde);
}

// row / col: (lse_s, lse_t, w, tw, hw) of the side.
int g_entry(uintptr_t stream, const void* zimg, const void* ztxt,
            const void* tprime, const Teacher& te, const void* tprime_t,
            const void* const (&rp)[5], const void* const (&cp)[5], void* g,
            void* gs_ws, int b, int n, int d, int d_t, long long ldg,
            int diag) {
  if (!dims_ok(zimg, ztxt, tprime, te, tprime_t, b, n, d, d_t) ||
      g == nullptr || gs_ws == nullptr || ldg < n)
    return (int)hipErrorInvalidValue;
  if (side_state(rp, 5) < 0 || side_state(cp, 5) < 0 ||
      (uintptr_t)gs_ws % 4 != 0 || (uintptr_t)g % 2 != 0)
    return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  const SideVecs rv{(const float*)rp[0], (const float*)rp[1],
                    (const float*)rp[2], (const float*)rp[3],
                    (const float*)rp[4]};
  const SideVecs cv{(const float*)cp[0], (const float*)cp[1],
                    (const float*)cp[2], (const float*)cp[3],
                    (const float*)cp[4]};
  if (te.mx)
    launch_g<mx_e4m3>((hipStream_t)stream, zimg, ztxt, tprime, te, tprime_t,
                      rv, cv, g, gs_ws, b, n, d, d_t, ldg, diag, tiles_m,
                      tiles_n);
  else
    launch_g<__bf16>((hipStream_t)stream, zimg, ztxt, tprime, te, tprime_t, rv,
                     cv, g, gs_ws, b, n, d, d_t, ldg, diag, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// Edge of the square output tile: workspaces are sized by ceil(b / tile) and
// ceil(n / tile).
int softmax_distill_tile_dim() { return BM; }

// Per row and per column of the (b, n) block: the student's LSE (z =
// exp(*tprime)·<zimg_i, ztxt_j>), the teacher's (v = exp(*tprime_t)·<timg_i,
// ttxt_j>) and x = Σ softmax(v)·(v − z), all fp32.  zimg (b, d), ztxt (n, d),
// timg (b, d_t), ttxt (n, d_t): bf16 row-major contiguous, d and d_t positive
// multiples of 8; tprime, tprime_t: device fp32.  row_ws / col_ws are
// workspaces of ceil(n/128)·b and ceil(b/128)·n 32-byte records.  A side
// whose workspace and three outputs are all null is skipped.  Returns
// non-zero, launching nothing, on anything unsupported.
int softmax_distill_stats_bf16(uintptr_t stream, const void* zimg,
                               const void* ztxt, const void* tprime,
                               const void* timg, const void* ttxt,
                               const void* tprime_t, void* row_ws,
                               void* col_ws, void* row_lse_s, void* row_lse_t,
                               void* row_x, void* col_lse_s, void* col_lse_t,
                               void* col_x, int b, int n, int d, int d_t) {
  return stats_entry(stream, zimg, ztxt, tprime,
                     Teacher{timg, ttxt, nullptr, nullptr, 0, false}, tprime_t,
                     row_ws, col_ws, row_lse_s, row_lse_t, row_x, col_lse_s,
                     col_lse_t, col_x, b, n, d, d_t);
}

// The same with an MXFP8 teacher pair: timg_q (b, d_t), ttxt_q (n, d_t) OCP
// e4m3fn bytes, row-major contiguous, d_t a multiple of 32; timg_e8 (b rows),
// ttxt_e8 (n rows) their e8m0 block scales, byte kb of a row for elements
// 32·kb … +31, 4-byte aligned with rows lde bytes apart, exactly
// 4·ceil(d_t / 128).  v is exp(*tprime_t) times the true dot of the
// dequantised values: tprime_t is passed unchanged.
int softmax_distill_stats_mxt(uintptr_t stream, const void* zimg,
                              const void* ztxt, const void* tprime,
                              const void* timg_q, const void* timg_e8,
                              const void* ttxt_q, const void* ttxt_e8,
                              const void* tprime_t, void* row_ws, void* col_ws,
                              void* row_lse_s, void* row_lse_t, void* row_x,
                              void* col_lse_s, void* col_lse_t, void* col_x,
                              int b, int n, int d, int d_t, long long lde) {
  return stats_entry(stream, zimg, ztxt, tprime,
                     Teacher{timg_q, ttxt_q, timg_e8, ttxt_e8, lde, true},
                     tprime_t, row_ws, col_ws, row_lse_s, row_lse_t, row_x,
                     col_lse_s, col_lse_t, col_x, b, n, d, d_t);
}

// g (b, n) bf16 with row stride ldg elements, and gs_ws[tile] = Σ g_ij·s_ij
// over each of the ceil(b/128)·ceil(n/128) tiles (row-major tile order).
// Per side lse_s, lse_t, w, tw, hw: fp32 vectors, all five or none; a side
// without them contributes nothing.  diag == INT_MIN: no hard positive.
int softmax_distill_g_bf16(uintptr_t stream, const void* zimg,
                           const void* ztxt, const void* tprime,
                           const void* timg, const void* ttxt,
                           const void* tprime_t, const void* row_lse_s,
                           const void* row_lse_t, const void* row_w,
                           const void* row_tw, const void* row_hw,
                           const void* col_lse_s, const void* col_lse_t,
                           const void* col_w, const void* col_tw,
                           const void* col_hw, void* g, void* gs_ws, int b,
                           int n, int d, int d_t, long long ldg, int diag) {
  const void* const rp[5] = {row_lse_s, row_lse_t, row_w, row_tw, row_hw};
  const void* const cp[5] = {col_lse_s, col_lse_t, col_w, col_tw, col_hw};
  return g_entry(stream, zimg, ztxt, tprime,
                 Teacher{timg, ttxt, nullptr, nullptr, 0, false}, tprime_t, rp,
                 cp, g, gs_ws, b, n, d, d_t, ldg, diag);
}

// The same with the MXFP8 teacher pair of softmax_distill_stats_mxt.
int softmax_distill_g_mxt(uintptr_t stream, const void* zimg,
                          const void* ztxt, const void* tprime,
                          const void* timg_q, const void* timg_e8,
                          const void* ttxt_q, const void* ttxt_e8,
                          const void* tprime_t, const void* row_lse_s,
                          const void* row_lse_t, const void* row_w,
                          const void* row_tw, const void* row_hw,
                          const void* col_lse_s, const void* col_lse_t,
                          const void* col_w, const void* col_tw,
                          const void* col_hw, void* g, void* gs_ws, int b,
                          int n, int d, int d_t, long long lde, long long ldg,
                          int diag) {
  const void* const rp[5] = {row_lse_s, row_lse_t, row_w, row_tw, row_hw};
  const void* const cp[5] = {col_lse_s, col_lse_t, col_w, col_tw, col_hw};
  return g_entry(stream, zimg, ztxt, tprime,
                 Teacher{timg_q, ttxt_q, timg_e8, ttxt_e8, lde, true},
                 tprime_t, rp, cp, g, gs_ws, b, n, d, d_t, ldg, diag);
}

}  // extern "C"
