// Sigmoid contrastive loss with sample-ID labels for gfx950 (MI355X): what a
// positive pair is comes from two int64 id vectors instead of the position,
// so a batch may hold several positives per row, none, repeated samples that
// must not count as negatives, and padding rows that count for nothing.
//
//   s_ij = <zimg_i, ztxt_j>   z_ij = t·s_ij + bias,  t = exp(t')
//   masked   : img_ids[i] < 0 or txt_ids[j] < 0
//   positive : ids equal                        (mode 0, "positive")
//              j == i + diag                    (mode 1, "ignore"; a pair with
//                                                equal ids off that diagonal
//                                                is masked as well)
//   negative : everything else
//   x = −l·z (l = ±1)   term = softplus(x)   g = −l·σ(x)      (0 where masked)
//
// One kernel template <WRITE_G>.  Both instantiations leave three fp32
// partials per 128×128 tile — Σ term, Σ g·s, Σ g — in a (tiles, 3) workspace;
// WRITE_G = true also stages the bf16 g tile in LDS and writes it as
// coalesced 16-byte row segments into a (b, n) view of row stride ldg.
// WRITE_G = false has no staging and no stores to g.  The partials of the
// two are bit-identical: the arithmetic is the same sequence of explicit
// fmas, and every reduction has a fixed order (xor shuffles, then the four
// waves in wave order).  No atomics, no counters.
//
// Structure.  The tile, its main loop (text fragment first: lane l owns image
// row (l & 15) and the four consecutive text columns 4·(l >> 4) … +3 of each
// fragment), the block walk, the id staging and the g
// write-out are pair_tile.h's; this file adds the epilogue.
//
// Ids.  Once the K loop's last barrier has passed, the tile's 128 row ids and
// 128 column ids are staged as int64 (pair_tile.h's stage_ids) in the 2 KiB
// above the g staging area; a row or column outside the block gets id −1
// there, so padding is masked by the same test as a negative id.  The mask
// matters: a zero-filled padding element has z = bias, not 0, and would add
// softplus(bias) to the loss.  The epilogue walks the fragments column-major,
// so a lane keeps its 4 row ids in registers and reads the 4 column ids of
// one fragment at a time.
//
// exp / log are the bare v_exp_f32 / v_log_f32 (base 2) with the ln 2 factors
// folded in; 1 / (1 + e) is v_rcp_f32 (1 ulp, 2⁻¹⁶ of a bf16 ulp).

#include "pair_tile.h"

namespace {

constexpr int IDS_OFF = G_STAGE_BYTES;        // 128 row ids, 128 column ids
constexpr int RED_OFF = IDS_OFF + IDS_BYTES;  // 4 waves × 3 partials

static_assert(IDS_OFF % 16 == 0, "id staging must take 16-byte reads");
static_assert(RED_OFF + 64 <= 2 * BUF_BYTES, "epilogue staging exceeds LDS");

template <bool WRITE_G>
__launch_bounds__(NTHREADS) __global__ void sigmoid_ids_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const float* __restrict__ bias,
    const long long* __restrict__ img_ids,
    const long long* __restrict__ txt_ids, __bf16* __restrict__ g,
    float* __restrict__ ws, int b, int n, int d, long long ldg, int diag,
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
  const float t = expf(tprime[0]);
  const float bs = bias[0];
  const bool ignore = ignore_dups != 0;

  long long* idl = reinterpret_cast<long long*>(lds + IDS_OFF);
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

  float s_loss = 0.f, s_gs = 0.f, s_g = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int lcol0 = wn * 64 + j * 16 + fq * 4;
    const int col0 = n0 + lcol0;
    long long cid[4];
    load_col_ids(idl, lcol0, cid);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x4 out;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = acc[i][j][r];
        const bool eq = rid[i] == cid[r];
        const bool on_diag = col0 + r == pc[i];
        const bool pos = ignore ? on_diag : eq;
        const bool masked = rid[i] < 0 || cid[r] < 0 ||
                            (ignore && eq && !on_diag);
        const float z = __builtin_fmaf(s, t, bs);
        const float x = pos ? -z : z;                  // −l·z
        const float e = __builtin_amdgcn_exp2f(-__builtin_fabsf(x) * LOG2E);
        const float den = 1.f + e;
        float term = __builtin_fmaf(LN2, __builtin_amdgcn_logf(den),
                                    __builtin_fmaxf(x, 0.f));
        const float sig = (x >= 0.f ? 1.f : e) * __builtin_amdgcn_rcpf(den);
        float gv = pos ? -sig : sig;                   // −l·σ(−l·z)
        if (masked) {
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

  if (!WRITE_G) return;

  store_g_tile(lds, g, ldg, m0, n0, b, n);
}

}  // namespace

extern "C" {

// Edge of the square output tile: the partials workspace holds
// ceil(b / tile)·ceil(n / tile) triples.
int sigmoid_ids_tile_dim() { return BM; }

// Sample-ID sigmoid loss over the (b, n) block of zimg (b, d) × ztxt (n, d),
// bf16 row-major contiguous; tprime, bias: device fp32 scalars; img_ids (b),
// txt_ids (n): device int64.  ws[tile] = (Σ term, Σ g·s, Σ g) per tile in
// row-major tile order.  g: null for the loss-only forward, otherwise a
// (b, n) bf16 view with row stride ldg elements.  diag == INT_MIN: no
// positional positive; it is read only when mode == 1 ("ignore"), mode == 0
// is "positive".  Returns non-zero, launching nothing, on anything
// unsupported.
int sigmoid_ids_bf16(uintptr_t stream, const void* zimg, const void* ztxt,
                     const void* tprime, const void* bias,
                     const void* img_ids, const void* txt_ids, void* g,
                     void* ws, int b, int n, int d, long long ldg, int diag,
                     int mode) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d) || tprime == nullptr ||
      bias == nullptr || img_ids == nullptr || txt_ids == nullptr ||
      ws == nullptr || (mode != 0 && mode != 1))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)img_ids | (uintptr_t)txt_ids) % 8 != 0 ||
      ((uintptr_t)tprime | (uintptr_t)bias | (uintptr_t)ws) % 4 != 0 ||
      (uintptr_t)g % 2 != 0)
    return (int)hipErrorInvalidValue;
  if (g != nullptr && ldg < n) return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (!pair_grid_ok(tiles_m, tiles_n)) return (int)hipErrorInvalidValue;
  const dim3 grid(tiles_m * tiles_n), block(NTHREADS);
  if (g != nullptr)
    hipLaunchKernelGGL(sigmoid_ids_kernel<true>, grid, block, 0,
                       (hipStream_t)stream, (const __bf16*)zimg,
                       (const __bf16*)ztxt, (const float*)tprime,
                       (const float*)bias, (const long long*)img_ids,
                       (const long long*)txt_ids, (__bf16*)g, (float*)ws, b,
                       n, d, ldg, diag, mode, tiles_m, tiles_n);
  else
    hipLaunchKernelGGL(sigmoid_ids_kernel<false>, grid, block, 0,
                       (hipStream_t)stream, (const __bf16*)zimg,
                       (const __bf16*)ztxt, (const float*)tprime,
                       (const float*)bias, (const long long*)img_ids,
                       (const long long*)txt_ids, (__bf16*)nullptr,
                       (float*)ws, b, n, d, ldg, diag, mode, tiles_m,
                       tiles_n);
  return (int)hipGetLastError();
}

}  // extern "C"
