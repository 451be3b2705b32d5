// Softmax (InfoNCE / CLIP) contrastive loss with sample-ID labels for gfx950
// (MI355X): the positives of a row or column come from two int64 id vectors,
// so a row may have several positives anywhere in the block, or none, pairs
// may count for nothing, and padding rows stay out of every normaliser.
//
//   s_ij = <zimg_i, ztxt_j>   z_ij = t·s_ij,  t = exp(t')
//   masked   : img_ids[i] < 0 or txt_ids[j] < 0
//   positive : ids equal                        (mode 0, "positive")
//              j == i + diag                    (mode 1, "ignore"; a pair with
//                                                equal ids off that diagonal
//                                                is masked as well)
//   A masked pair is never a positive.
//   row_lse_i = log Σ_{j not masked} exp(z_ij)   (−inf for a fully masked row)
//   row_pos_i = Σ_{j positive} z_ij     row_cnt_i = #{j positive}
//   (columns alike, over i)
//   g_ij = 0 where masked, otherwise
//          row_w_i·exp(z_ij − row_lse_i) + col_w_j·exp(z_ij − col_lse_j)
//          − [positive]·(row_pw_i + col_pw_j)
//
// Three kernels:
//
// - softmax_ids_partials_kernel: per 128×128 tile, each row's
//   (max, Σ exp(z − max)) over the tile's unmasked columns, the sum of its
//   positive logits and their count, and the same per column over the tile's
//   rows, written as 16-byte records to workspaces laid out (tiles_n, b) and
//   (tiles_m, n).  `max` is in units of z.
// - softmax_ids_finish_kernel: one thread per row / column folds its tile
//   partials in tile order: lse = M + log Σ_t sum_t·exp(max_t − M), the
//   positive sums in fp32, the counts as integers.
// - softmax_ids_g_kernel: the same main loop and classes; the epilogue
//   evaluates g from the fp32 LSE and weight vectors, stages the bf16 tile in
//   LDS and writes it as coalesced 16-byte row segments into a (b, n) view of
//   row stride ldg, and leaves one fp32 partial Σ g_ij·s_ij per tile.
//
// There is no atomic and no counter anywhere: every reduction has a fixed
// order (xor shuffles, the two or four waves in wave order, tiles in tile
// order), so all results are bitwise reproducible.
//
// Structure.  The tile, its main loop (text fragment first: lane l owns image
// row (l & 15) and the four consecutive text columns 4·(l >> 4) … +3 of each
// fragment), the block walk, the id staging and the g
// write-out are pair_tile.h's; this file adds the epilogues.
//
// Ids.  Once the K loop's last barrier has passed, the tile's 128 row ids and
// 128 column ids are staged as int64 in LDS (stage_ids); a row or column
// outside the block gets id −1 there, so padding is masked by the same test
// as a negative id.  The epilogues walk the fragments column-major, so a lane
// keeps its 4 row ids in registers and reads the 4 column ids of one fragment
// at a time.
//
// Masking.  A masked element becomes −inf before the max and the sum, by a
// select; a partial over masked elements alone is (−inf, 0) with positive
// sum 0 and count 0, and the subtraction of the max is guarded so that it
// never forms inf − inf.  In the g kernel a masked row has lse = −inf, the
// unselected value there is 0·inf, and the select after it makes g exactly 0.
//
// exp / log are the bare v_exp_f32 / v_log_f32 (base 2) with the ln 2 factors
// folded into the scale of the argument and of the result.

#include "pair_tile.h"

namespace {

// Partials kernel: ids, then the two waves' records of each row and column.
struct __attribute__((aligned(16))) Partial {
  float m;     // max of the unmasked logits (raw dots in LDS, ·t in memory)
  float s;     // Σ exp(z − max)
  float pos;   // Σ of the positive logits (raw dots in LDS, ·t in memory)
  int cnt;     // number of positives
};
static_assert(sizeof(Partial) == 16, "one 16-byte store per record");

constexpr int LSE_IDS_OFF = 0;
constexpr int LSE_PART_OFF = LSE_IDS_OFF + IDS_BYTES;  // 2·(BM + BN) records
static_assert(LSE_PART_OFF % 16 == 0, "records take 16-byte accesses");
static_assert(LSE_PART_OFF + 2 * (BM + BN) * (int)sizeof(Partial)
                  <= 2 * BUF_BYTES, "epilogue staging exceeds LDS");

// g kernel: the g staging tile, then the ids, then 4 waves × 1 partial.
constexpr int G_IDS_OFF = G_STAGE_BYTES;
constexpr int G_RED_OFF = G_IDS_OFF + IDS_BYTES;
static_assert(G_IDS_OFF % 16 == 0, "id staging must take 16-byte reads");
static_assert(G_RED_OFF + 16 <= 2 * BUF_BYTES, "epilogue staging exceeds LDS");

// Two waves per SIMD asked for: two workgroups share a CU (64 KiB of LDS
// each), which is 256 registers per lane; left alone the scheduler spends
// more on the epilogue's shuffles and halves the occupancy.
__launch_bounds__(NTHREADS, 2) __global__ void softmax_ids_partials_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const long long* __restrict__ img_ids,
    const long long* __restrict__ txt_ids, Partial* __restrict__ row_ws,
    Partial* __restrict__ col_ws, int b, int n, int d, int diag,
    int ignore_dups, int tiles_m, int tiles_n) {
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
  const bool ignore = ignore_dups != 0;

  long long* idl = reinterpret_cast<long long*>(lds + LSE_IDS_OFF);
  stage_ids(idl, img_ids, txt_ids, m0, n0, b, n);

  // This lane's four rows: id, and the column of the row's positional
  // positive ("ignore" only; −1 when it has none inside the block).
  long long rid[4];
  int pc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lrow = wm * 64 + i * 16 + fr;
    rid[i] = idl[lrow];
    pc[i] = positive_col(m0 + lrow, ignore ? diag : DIAG_NONE, n);
  }

  // Classes: a masked element (padding included: its id is −1) becomes −inf;
  // an unmasked positive adds its dot and 1 to its row and to its column.
  float rpos[4] = {0.f, 0.f, 0.f, 0.f};
  int rcnt[4] = {0, 0, 0, 0};
  // part_row[wn][128], part_col[wm][128]; m and pos of raw dots.
  Partial* part_row = reinterpret_cast<Partial*>(lds + LSE_PART_OFF);
  Partial* part_col = part_row + 2 * BM;

  // Fragment column by fragment column: a fragment's four columns are
  // complete in this wave once its four rows are through, so they are
  // reduced right away and only the row sums are carried.
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int lcol0 = wn * 64 + j * 16 + fq * 4;
    long long cid[4];
    load_col_ids(idl, lcol0, cid);
    float cpos[4] = {0.f, 0.f, 0.f, 0.f};
    int ccnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[i][j][r];
        const bool eq = rid[i] == cid[r];
        const bool on_diag = n0 + lcol0 + r == pc[i];
        const bool masked = rid[i] < 0 || cid[r] < 0 ||
                            (ignore && eq && !on_diag);
        const bool pos = (ignore ? on_diag : eq) && !masked;
        const float ps = pos ? s : 0.f;
        const int pn = pos ? 1 : 0;
        rpos[i] += ps;
        rcnt[i] += pn;
        cpos[r] += ps;
        ccnt[r] += pn;
        acc[i][j][r] = masked ? -inf : s;
      }
    if (cols_on) {
      // A column lives in the 16 lanes that share fq (lane bits 0-3).
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
        float ps = cpos[r];
        int pn = ccnt[r];
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) {
          s += __shfl_xor(s, x, 64);
          ps += __shfl_xor(ps, x, 64);
          pn += __shfl_xor(pn, x, 64);
        }
        if (fr == 0) part_col[wm * BN + lcol0 + r] = Partial{m, s, ps, pn};
      }
    }
  }

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
      float ps = rpos[i];
      int pn = rcnt[i];
      s += __shfl_xor(s, 16, 64);
      ps += __shfl_xor(ps, 16, 64);
      pn += __shfl_xor(pn, 16, 64);
      s += __shfl_xor(s, 32, 64);
      ps += __shfl_xor(ps, 32, 64);
      pn += __shfl_xor(pn, 32, 64);
      if (fq == 0)
        part_row[wn * BM + wm * 64 + i * 16 + fr] = Partial{m, s, ps, pn};
    }
  }
  __syncthreads();

  // Fold the two waves of each row / column (wave 0 first) and store.
  const bool row_half = tid < BM;
  const int e = row_half ? tid : tid - BM;
  if (row_half ? !rows_on : !cols_on) return;
  const Partial* part = row_half ? part_row : part_col;
  const Partial p0 = part[e], p1 = part[BM + e];
  const float m = fmaxf(p0.m, p1.m);
  const float ms = safe_max(m);
  const float s = p0.s * __builtin_amdgcn_exp2f((p0.m - ms) * sc2) +
                  p1.s * __builtin_amdgcn_exp2f((p1.m - ms) * sc2);
  const Partial out{m * t, s, (p0.pos + p1.pos) * t, p0.cnt + p1.cnt};
  if (row_half) {
    if (m0 + e < b) row_ws[(long long)tp.tn * b + (m0 + e)] = out;
  } else {
    if (n0 + e < n) col_ws[(long long)tp.tm * n + (n0 + e)] = out;
  }
}

// One thread per row (ids 0 … b−1, when row_lse is given) or column (the
// ids after them): fold `tiles` partials, tile 0 first.
__launch_bounds__(NTHREADS) __global__ void softmax_ids_finish_kernel(
    const Partial* __restrict__ row_ws, const Partial* __restrict__ col_ws,
    float* __restrict__ row_lse, float* __restrict__ row_pos,
    int* __restrict__ row_cnt, float* __restrict__ col_lse,
    float* __restrict__ col_pos, int* __restrict__ col_cnt, int b, int n,
    int tiles_m, int tiles_n) {
  const long long id = (long long)blockIdx.x * NTHREADS + threadIdx.x;
  const long long nrows = row_lse != nullptr ? b : 0;
  const long long ncols = col_lse != nullptr ? n : 0;
  const Partial* ws;
  float *lse, *pos;
  int* cnt;
  long long len, e;
  int tiles;
  if (id < nrows) {
    ws = row_ws; lse = row_lse; pos = row_pos; cnt = row_cnt;
    len = b; e = id; tiles = tiles_n;
  } else if (id - nrows < ncols) {
    ws = col_ws; lse = col_lse; pos = col_pos; cnt = col_cnt;
    len = n; e = id - nrows; tiles = tiles_m;
  } else {
    return;
  }
  float m = -__builtin_inff();
  for (int k = 0; k < tiles; ++k) m = fmaxf(m, ws[k * len + e].m);
  const float ms = safe_max(m);
  float s = 0.f, ps = 0.f;
  int pn = 0;
  for (int k = 0; k < tiles; ++k) {
    const Partial p = ws[k * len + e];
    s += p.s * __builtin_amdgcn_exp2f((p.m - ms) * LOG2E);
    ps += p.pos;
    pn += p.cnt;
  }
  // Nothing unmasked: m = −inf and s = 0, the sum of two −inf.
  lse[e] = m + LN2 * __builtin_amdgcn_logf(s);
  pos[e] = ps;
  cnt[e] = pn;
}

__launch_bounds__(NTHREADS) __global__ void softmax_ids_g_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const long long* __restrict__ img_ids,
    const long long* __restrict__ txt_ids, const float* __restrict__ row_lse,
    const float* __restrict__ row_w, const float* __restrict__ row_pw,
    const float* __restrict__ col_lse, const float* __restrict__ col_w,
    const float* __restrict__ col_pw, __bf16* __restrict__ g,
    float* __restrict__ gs_ws, int b, int n, int d, long long ldg, int diag,
    int ignore_dups, int tiles_m, int tiles_n) {
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
  const bool ignore = ignore_dups != 0;

  long long* idl = reinterpret_cast<long long*>(lds + G_IDS_OFF);
  stage_ids(idl, img_ids, txt_ids, m0, n0, b, n);

  // This lane's four rows: id, positional positive, −row_lse·log2 e, row_w
  // and row_pw (0 outside the block and for a skipped side).
  long long rid[4];
  int pc[4];
  float rl2[4], rw[4], rpw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lrow = wm * 64 + i * 16 + fr;
    const int row = m0 + lrow;
    const bool on = rows_on && row < b;
    rid[i] = idl[lrow];
    pc[i] = positive_col(row, ignore ? diag : DIAG_NONE, n);
    rl2[i] = on ? -row_lse[row] * LOG2E : 0.f;
    rw[i] = on ? row_w[row] : 0.f;
    rpw[i] = on ? row_pw[row] : 0.f;
  }

  float s_gs = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int lcol0 = wn * 64 + j * 16 + fq * 4;
    const int col0 = n0 + lcol0;
    long long cid[4];
    load_col_ids(idl, lcol0, cid);
    float cl2[4], cw[4], cpw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = cols_on && col0 + r < n;
      cl2[r] = on ? -col_lse[col0 + r] * LOG2E : 0.f;
      cw[r] = on ? col_w[col0 + r] : 0.f;
      cpw[r] = on ? col_pw[col0 + r] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x4 out;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[i][j][r];
        const bool eq = rid[i] == cid[r];
        const bool on_diag = col0 + r == pc[i];
        const bool masked = rid[i] < 0 || cid[r] < 0 ||
                            (ignore && eq && !on_diag);
        const bool pos = ignore ? on_diag : eq;
        // A skipped side adds no term at all (never 0 · exp(…)).
        float gv = 0.f;
        if (rows_on)
          gv += rw[i] * __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, rl2[i]));
        if (cols_on)
          gv += cw[r] * __builtin_amdgcn_exp2f(__builtin_fmaf(s, sc2, cl2[r]));
        if (pos) gv -= rpw[i] + cpw[r];
        // A select: a fully masked row or column has lse = −inf and the
        // value above is 0 · inf there.
        gv = masked ? 0.f : gv;
        s_gs += gv * s;
        out[r] = (__bf16)gv;
      }
      *reinterpret_cast<bf16x4*>(lds + (wm * 64 + i * 16 + fr) * G_PITCH
                                 + 2 * lcol0) = out;
    }
  }

  // Σ g·s of the tile: lanes by xor shuffles, then the four waves in order.
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) s_gs += __shfl_xor(s_gs, x, 64);
  float* red = reinterpret_cast<float*>(lds + G_RED_OFF);
  if (lane == 0) red[wave] = s_gs;
  __syncthreads();
  if (tid == 0)
    gs_ws[(long long)tp.tm * tiles_n + tp.tn] =
        ((red[0] + red[1]) + red[2]) + red[3];

  store_g_tile(lds, g, ldg, m0, n0, b, n);
}

// The embedding checks plus what both entries add: t', the ids, the mode and
// the grid size.
bool dims_ok(const void* zimg, const void* ztxt, const void* tprime,
             const void* img_ids, const void* txt_ids, int b, int n, int d,
             int mode) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d) || tprime == nullptr ||
      (uintptr_t)tprime % 4 != 0)
    return false;
  if (img_ids == nullptr || txt_ids == nullptr ||
      ((uintptr_t)img_ids | (uintptr_t)txt_ids) % 8 != 0)
    return false;
  if (mode != 0 && mode != 1) return false;
  return pair_grid_ok(ceil_div(b, BM), ceil_div(n, BN));
}

}  // namespace

extern "C" {

// Edge of the square output tile: workspaces are sized by ceil(b / tile) and
// ceil(n / tile).
int softmax_ids_tile_dim() { return BM; }

// Masked LSE, positive-logit sum and positive count of every row and column
// of the (b, n) block of zimg (b, d) × ztxt (n, d), bf16 row-major
// contiguous, with z = exp(*tprime)·<·,·> (tprime: device fp32); img_ids (b),
// txt_ids (n): device int64.  row_ws / col_ws are workspaces of
// ceil(n/128)·b and ceil(b/128)·n 16-byte records.  lse, pos: fp32; cnt:
// int32.  A side whose workspace and three outputs are all null is skipped.
// diag == INT_MIN: no positional positive; it is read only when mode == 1
// ("ignore"), mode == 0 is "positive".  Returns non-zero, launching nothing,
// on anything unsupported.
int softmax_ids_lse_bf16(uintptr_t stream, const void* zimg, const void* ztxt,
                         const void* tprime, const void* img_ids,
                         const void* txt_ids, void* row_ws, void* col_ws,
                         void* row_lse, void* row_pos, void* row_cnt,
                         void* col_lse, void* col_pos, void* col_cnt, int b,
                         int n, int d, int diag, int mode) {
  if (!dims_ok(zimg, ztxt, tprime, img_ids, txt_ids, b, n, d, mode))
    return (int)hipErrorInvalidValue;
  const bool rows = row_ws != nullptr, cols = col_ws != nullptr;
  if ((row_lse != nullptr) != rows || (row_pos != nullptr) != rows ||
      (row_cnt != nullptr) != rows || (col_lse != nullptr) != cols ||
      (col_pos != nullptr) != cols || (col_cnt != nullptr) != cols)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)row_ws | (uintptr_t)col_ws) % 16 != 0 ||
      ((uintptr_t)row_lse | (uintptr_t)row_pos | (uintptr_t)row_cnt |
       (uintptr_t)col_lse | (uintptr_t)col_pos | (uintptr_t)col_cnt) % 4 != 0)
    return (int)hipErrorInvalidValue;
  if (!rows && !cols) return 0;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  hipLaunchKernelGGL(softmax_ids_partials_kernel, dim3(tiles_m * tiles_n),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt,
                     (const float*)tprime, (const long long*)img_ids,
                     (const long long*)txt_ids, (Partial*)row_ws,
                     (Partial*)col_ws, b, n, d, diag, mode, tiles_m, tiles_n);
  int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  const long long ids = (rows ? (long long)b : 0) + (cols ? (long long)n : 0);
  hipLaunchKernelGGL(softmax_ids_finish_kernel,
                     dim3((unsigned)((ids + NTHREADS - 1) / NTHREADS)),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const Partial*)row_ws, (const Partial*)col_ws,
                     (float*)row_lse, (float*)row_pos, (int*)row_cnt,
                     (float*)col_lse, (float*)col_pos, (int*)col_cnt, b, n,
                     tiles_m, tiles_n);
  return (int)hipGetLastError();
}

// g (b, n) bf16 with row stride ldg elements, and gs_ws[tile] = Σ g_ij·s_ij
// over each of the ceil(b/128)·ceil(n/128) tiles (row-major tile order).
// Per side lse, w, pw: fp32 vectors, all three or none; a side without them
// contributes nothing.  Ids, diag and mode as above.
int softmax_ids_g_bf16(uintptr_t stream, const void* zimg, const void* ztxt,
                       const void* tprime, const void* img_ids,
                       const void* txt_ids, const void* row_lse,
                       const void* row_w, const void* row_pw,
                       const void* col_lse, const void* col_w,
                       const void* col_pw, void* g, void* gs_ws, int b, int n,
                       int d, long long ldg, int diag, int mode) {
  if (!dims_ok(zimg, ztxt, tprime, img_ids, txt_ids, b, n, d, mode) ||
      g == nullptr || gs_ws == nullptr || ldg < n)
    return (int)hipErrorInvalidValue;
  const bool rows = row_lse != nullptr, cols = col_lse != nullptr;
  if ((row_w != nullptr) != rows || (row_pw != nullptr) != rows ||
      (col_w != nullptr) != cols || (col_pw != nullptr) != cols)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)row_lse | (uintptr_t)row_w | (uintptr_t)row_pw |
       (uintptr_t)col_lse | (uintptr_t)col_w | (uintptr_t)col_pw |
       (uintptr_t)gs_ws) % 4 != 0 ||
      (uintptr_t)g % 2 != 0)
    return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  hipLaunchKernelGGL(softmax_ids_g_kernel, dim3(tiles_m * tiles_n),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt,
                     (const float*)tprime, (const long long*)img_ids,
                     (const long long*)txt_ids, (const float*)row_lse,
                     (const float*)row_w, (const float*)row_pw,
                     (const float*)col_lse, (const float*)col_w,
                     (const float*)col_pw, (__bf16*)g, (float*)gs_ws, b, n, d,
                     ldg, diag, mode, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

}  // extern "C"
