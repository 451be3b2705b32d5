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
// One tile body template <GFMT, OP>, three kernels on bf16 operands (two
// more on e4m3 operands, below).  All leave three fp32
// partials per 128×128 tile — Σ term, Σ g·s, Σ g — in a (tiles, 3) workspace;
// G_BF16 also stages the bf16 g tile in LDS and writes it as coalesced
// 16-byte row segments into a (b, n) view of row stride ldg; G_NONE has no
// staging and no stores to g; G_E4M3 writes g as a (b, n) e4m3 slab and gᵀ
// as an (n, b) e4m3 slab (below).  The partials of the three are
// bit-identical: they come from the fp32 g, the arithmetic is the same
// sequence of explicit fmas, and every reduction has a fixed order (xor
// shuffles, then the four waves in wave order).  No atomics, no counters.
//
// The e4m3 slab pair (the `mixed` policy: exact bf16 logits, fp8 gradient
// GEMMs).  Both slabs hold the OCP e4m3fn code of 448·g, the encoding of
// siglip_kernels.hip's pair; a masked or padding pair is byte 0x00.  A lane's
// four values of a fragment are four consecutive bytes of one g row: one
// packed dword, one 4-byte LDS write.  gᵀ wants four consecutive rows of one
// column: lanes fr = 4a … 4a+3 are a DPP quad and hold a 4×4 byte block,
// which pair_tile.h's quad_transpose_bytes turns in place (2 DPP moves, 2
// v_perm_b32), so lane fr & 3 = c holds column 4·fq + c, rows 4a … 4a+3, and
// does one 4-byte write into a [column][row] tile.  16 dword writes per slab
// per lane, one staging barrier (the reduction's), two coalesced write-outs
// (store_g8_tile).  The two tiles take 36 KiB; ids and reduction slots sit
// above them.  This kernel is compiled without packed fp32 instructions.
//
// e4m3 operands (the `fp8` policy).  The tile body takes the operand type as
// a second template parameter and calls pair_tile.h's e4m3 main loop
// (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales, half the K steps)
// instead of the bf16 one; everything after the K loop is the same code.  Two
// more kernels, sigmoid_ids_fp8_kernel<false> (G_NONE) and <true> (G_E4M3),
// both without packed fp32 instructions, so their partials agree bit for bit
// with each other (not with the bf16-operand kernels: other logits).  s is
// the raw dot of the e4m3 values and the per-tensor scales arrive folded into
// t'; row-wise scales are not built.
//
// MX operands (the `mxfp8` policy).  A third operand type, mx_e4m3: the same
// e4m3 bytes with one e8m0 scale per 32 consecutive k (OCP MXFP8), read by
// pair_tile.h's MX main loop, which stages the scale dwords next to the
// element slabs and hands each MFMA its lanes' block scales.  s is then the
// true dot of the dequantised values and t' arrives unchanged.  Two more
// kernels, sigmoid_ids_mx_kernel<false> (G_NONE) and <true> (G_E4M3), with
// 66 KiB of LDS (still two workgroups per CU) and without packed fp32
// instructions: with every scale byte 0x7F they leave the bits of the fp8
// pair.  Everything after the K loop is the same code.
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

#include <type_traits>

namespace {

enum { G_NONE = 0, G_BF16 = 1, G_E4M3 = 2 };

// 128 row ids and 128 column ids above the g staging, then 4 waves × 3
// partials.
constexpr int ids_off(int gfmt) {
  return gfmt == G_E4M3 ? 2 * G8_TILE_BYTES : G_STAGE_BYTES;
}
constexpr int red_off(int gfmt) { return ids_off(gfmt) + IDS_BYTES; }

static_assert(ids_off(G_BF16) % 16 == 0 && ids_off(G_E4M3) % 16 == 0,
              "id staging must take 16-byte reads");
static_assert(red_off(G_BF16) + 64 <= 2 * BUF_BYTES &&
                  red_off(G_E4M3) + 64 <= 2 * BUF_BYTES,
              "epilogue staging exceeds LDS");

// One tile: g is the bf16 slab (G_BF16) or the e4m3 slab (G_E4M3), gt the
// e4m3 transpose (G_E4M3 only).  OP is the operand element: __bf16, or
// unsigned char for e4m3 (s is then the raw dot of the e4m3 values and
// tprime holds the folded scales), or mx_e4m3 with the block scales in
// zimg_e8 / ztxt_e8, rows lde bytes apart (s is the true dot).  `lds` is the
// workgroup's 2 · BUF_BYTES, MX_LDS_BYTES for mx_e4m3.
template <int GFMT, typename OP = __bf16>
__device__ __forceinline__ void sigmoid_ids_tile(
    const OP* __restrict__ zimg, const OP* __restrict__ ztxt,
    const float* __restrict__ tprime, const float* __restrict__ bias,
    const long long* __restrict__ img_ids,
    const long long* __restrict__ txt_ids, void* __restrict__ g,
    void* __restrict__ gt, float* __restrict__ ws, int b, int n, int d,
    long long ldg, long long ldgt, int diag, int ignore_dups, int tiles_m,
    int tiles_n, unsigned char* lds,
    const unsigned char* __restrict__ zimg_e8 = nullptr,
    const unsigned char* __restrict__ ztxt_e8 = nullptr, int lde = 0) {
  constexpr int IDS_OFF = ids_off(GFMT), RED_OFF = red_off(GFMT);
  const TilePos tp = tile_of_block(tiles_m, tiles_n);
  const int m0 = tp.tm * BM, n0 = tp.tn * BN;
  f32x4 acc[4][4];
  if constexpr (std::is_same<OP, mx_e4m3>::value)
    pair_tile_dots_mx<true>((const unsigned char*)zimg, zimg_e8,
                            (const unsigned char*)ztxt, ztxt_e8, b, n, d, lde,
                            m0, n0, lds, acc);
  else if constexpr (sizeof(OP) == 1)
    pair_tile_dots_e4m3<true>(zimg, ztxt, b, n, d, m0, n0, lds, acc);
  else
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
      f32x4 gq;
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
        if (GFMT == G_BF16) out[r] = (__bf16)gv;
        if (GFMT == G_E4M3) gq[r] = gv;
      }
      if (GFMT == G_BF16)
        *reinterpret_cast<bf16x4*>(lds + (wm * 64 + i * 16 + fr) * G_PITCH
                                   + 2 * lcol0) = out;
      if (GFMT == G_E4M3) {
        // g: row fr, columns lcol0 … +3.  gᵀ after the quad transpose:
        // column lcol0 + (fr & 3), rows 4·(fr >> 2) … +3 of this fragment.
        const unsigned codes = pack_e4m3x4(gq);
        *reinterpret_cast<unsigned*>(lds + (wm * 64 + i * 16 + fr) * G8_PITCH
                                     + lcol0) = codes;
        *reinterpret_cast<unsigned*>(
            lds + G8_TILE_BYTES + (lcol0 + (fr & 3)) * G8_PITCH + wm * 64 +
            i * 16 + (fr & 12)) = quad_transpose_bytes(codes, fr & 3);
      }
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

  if (GFMT == G_BF16) store_g_tile(lds, (__bf16*)g, ldg, m0, n0, b, n);
  if (GFMT == G_E4M3) {
    store_g8_tile(lds, (unsigned char*)g, ldg, m0, n0, b, n);
    store_g8_tile(lds + G8_TILE_BYTES, (unsigned char*)gt, ldgt, n0, m0, n, b);
  }
}

template <bool WRITE_G>
__launch_bounds__(NTHREADS) __global__ void sigmoid_ids_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const float* __restrict__ bias,
    const long long* __restrict__ img_ids,
    const long long* __restrict__ txt_ids, __bf16* __restrict__ g,
    float* __restrict__ ws, int b, int n, int d, long long ldg, int diag,
    int ignore_dups, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];
  sigmoid_ids_tile<WRITE_G ? G_BF16 : G_NONE>(
      zimg, ztxt, tprime, bias, img_ids, txt_ids, g, nullptr, ws, b, n, d, ldg,
      0, diag, ignore_dups, tiles_m, tiles_n, lds);
}

__attribute__((target("no-packed-fp32-ops")))
__launch_bounds__(NTHREADS) __global__ void sigmoid_ids_e4m3_kernel(
    const __bf16* __restrict__ zimg, const __bf16* __restrict__ ztxt,
    const float* __restrict__ tprime, const float* __restrict__ bias,
    const long long* __restrict__ img_ids,
    const long long* __restrict__ txt_ids, unsigned char* __restrict__ g8,
    unsigned char* __restrict__ gt8, float* __restrict__ ws, int b, int n,
    int d, long long ldg, long long ldgt, int diag, int ignore_dups,
    int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];
  sigmoid_ids_tile<G_E4M3>(zimg, ztxt, tprime, bias, img_ids, txt_ids, g8, gt8,
                           ws, b, n, d, ldg, ldgt, diag, ignore_dups, tiles_m,
                           tiles_n, lds);
}

// e4m3 operands (the `fp8` policy): loss only (WRITE_G false; g8, gt8 unused)
// or the e4m3 slab pair.  Compiled without packed fp32 instructions, both, so
// that the two leave the same partials.
template <bool WRITE_G>
__attribute__((target("no-packed-fp32-ops")))
__launch_bounds__(NTHREADS) __global__ void sigmoid_ids_fp8_kernel(
    const unsigned char* __restrict__ zimg_q,
    const unsigned char* __restrict__ ztxt_q,
    const float* __restrict__ tprime, const float* __restrict__ bias,
    const long long* __restrict__ img_ids,
    const long long* __restrict__ txt_ids, unsigned char* __restrict__ g8,
    unsigned char* __restrict__ gt8, float* __restrict__ ws, int b, int n,
    int d, long long ldg, long long ldgt, int diag, int ignore_dups,
    int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];
  sigmoid_ids_tile<WRITE_G ? G_E4M3 : G_NONE, unsigned char>(
      zimg_q, ztxt_q, tprime, bias, img_ids, txt_ids, g8, gt8, ws, b, n, d,
      ldg, ldgt, diag, ignore_dups, tiles_m, tiles_n, lds);
}

// MX operands (the `mxfp8` policy): the fp8 pair's two forms with the e8m0
// block scales of both operands, one dword per row and 128-element K-step.
template <bool WRITE_G>
__attribute__((target("no-packed-fp32-ops")))
__launch_bounds__(NTHREADS) __global__ void sigmoid_ids_mx_kernel(
    const unsigned char* __restrict__ zimg_q,
    const unsigned char* __restrict__ zimg_e8,
    const unsigned char* __restrict__ ztxt_q,
    const unsigned char* __restrict__ ztxt_e8,
    const float* __restrict__ tprime, const float* __restrict__ bias,
    const long long* __restrict__ img_ids,
    const long long* __restrict__ txt_ids, unsigned char* __restrict__ g8,
    unsigned char* __restrict__ gt8, float* __restrict__ ws, int b, int n,
    int d, int lde, long long ldg, long long ldgt, int diag, int ignore_dups,
    int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[MX_LDS_BYTES];
  sigmoid_ids_tile<WRITE_G ? G_E4M3 : G_NONE, mx_e4m3>(
      (const mx_e4m3*)zimg_q, (const mx_e4m3*)ztxt_q, tprime, bias, img_ids,
      txt_ids, g8, gt8, ws, b, n, d, ldg, ldgt, diag, ignore_dups, tiles_m,
      tiles_n, lds, zimg_e8, ztxt_e8, lde);
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

// The same loss with dL/dlogit as an e4m3 slab pair: g8 a (b, n) view of row
// stride ldg bytes, gt8 an (n, b) view of row stride ldgt bytes, both the
// e4m3fn code of 448·g (0x00 where masked), any alignment.  Everything else,
// and ws bit for bit, as sigmoid_ids_bf16.  Returns non-zero, launching
// nothing, on anything unsupported.
int sigmoid_ids_e4m3(uintptr_t stream, const void* zimg, const void* ztxt,
                     const void* tprime, const void* bias,
                     const void* img_ids, const void* txt_ids, void* g8,
                     void* gt8, void* ws, int b, int n, int d, long long ldg,
                     long long ldgt, int diag, int mode) {
  if (!pair_dims_ok(zimg, ztxt, b, n, d) || tprime == nullptr ||
      bias == nullptr || img_ids == nullptr || txt_ids == nullptr ||
      ws == nullptr || g8 == nullptr || gt8 == nullptr ||
      (mode != 0 && mode != 1))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)img_ids | (uintptr_t)txt_ids) % 8 != 0 ||
      ((uintptr_t)tprime | (uintptr_t)bias | (uintptr_t)ws) % 4 != 0)
    return (int)hipErrorInvalidValue;
  if (ldg < n || ldgt < b) return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (!pair_grid_ok(tiles_m, tiles_n)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sigmoid_ids_e4m3_kernel, dim3(tiles_m * tiles_n),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const __bf16*)zimg, (const __bf16*)ztxt,
                     (const float*)tprime, (const float*)bias,
                     (const long long*)img_ids, (const long long*)txt_ids,
                     (unsigned char*)g8, (unsigned char*)gt8, (float*)ws, b, n,
                     d, ldg, ldgt, diag, mode, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

// The loss from e4m3 operands: zimg_q (b, d), ztxt_q (n, d) OCP e4m3fn bytes,
// row-major contiguous, d a multiple of 16.  s is the raw dot of the e4m3
// values and z = exp(*tprime)·s + bias, so the caller adds the logs of its
// per-tensor scales to t'; ws[tile] = (Σ term, Σ g·s, Σ g) in those units.
// g8 and gt8 both null: loss only; both given: the slab pair of
// sigmoid_ids_e4m3 (same views, same encoding); exactly one: an error.
// Returns non-zero, launching nothing, on anything unsupported.
int sigmoid_ids_fp8(uintptr_t stream, const void* zimg_q, const void* ztxt_q,
                    const void* tprime, const void* bias, const void* img_ids,
                    const void* txt_ids, void* g8, void* gt8, void* ws, int b,
                    int n, int d, long long ldg, long long ldgt, int diag,
                    int mode) {
  if (!pair_dims_ok_e4m3(zimg_q, ztxt_q, b, n, d) || tprime == nullptr ||
      bias == nullptr || img_ids == nullptr || txt_ids == nullptr ||
      ws == nullptr || (g8 == nullptr) != (gt8 == nullptr) ||
      (mode != 0 && mode != 1))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)img_ids | (uintptr_t)txt_ids) % 8 != 0 ||
      ((uintptr_t)tprime | (uintptr_t)bias | (uintptr_t)ws) % 4 != 0)
    return (int)hipErrorInvalidValue;
  if (g8 != nullptr && (ldg < n || ldgt < b)) return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (!pair_grid_ok(tiles_m, tiles_n)) return (int)hipErrorInvalidValue;
  const auto kernel = g8 != nullptr ? sigmoid_ids_fp8_kernel<true>
                                    : sigmoid_ids_fp8_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(tiles_m * tiles_n), dim3(NTHREADS), 0,
                     (hipStream_t)stream, (const unsigned char*)zimg_q,
                     (const unsigned char*)ztxt_q, (const float*)tprime,
                     (const float*)bias, (const long long*)img_ids,
                     (const long long*)txt_ids, (unsigned char*)g8,
                     (unsigned char*)gt8, (float*)ws, b, n, d, ldg, ldgt, diag,
                     mode, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

// The loss from MX operands: zimg_q (b, d), ztxt_q (n, d) OCP e4m3fn bytes,
// row-major contiguous, d a multiple of 32; zimg_e8 (b rows), ztxt_e8 (n
// rows) their e8m0 block scales, byte kb of a row for elements 32·kb … +31,
// 4-byte aligned with rows lde_img / lde_txt bytes apart, both exactly
// 4·ceil(d / 128) (bytes past d / 32 are not applied to anything: their
// elements are zero-filled).  s is the true dot Σ 2^(ea + eb − 254)·a·b and
// z = exp(*tprime)·s + bias.  Slabs, ws, labels and every other check as
// sigmoid_ids_fp8; with every scale byte 0x7F its bits.  Returns non-zero,
// launching nothing, on anything unsupported.
int sigmoid_ids_mx(uintptr_t stream, const void* zimg_q, const void* zimg_e8,
                   const void* ztxt_q, const void* ztxt_e8,
                   const void* tprime, const void* bias, const void* img_ids,
                   const void* txt_ids, void* g8, void* gt8, void* ws, int b,
                   int n, int d, long long lde_img, long long lde_txt,
                   long long ldg, long long ldgt, int diag, int mode) {
  if (!pair_dims_ok_mx(zimg_q, zimg_e8, ztxt_q, ztxt_e8, b, n, d, lde_img,
                       lde_txt) ||
      tprime == nullptr || bias == nullptr || img_ids == nullptr ||
      txt_ids == nullptr || ws == nullptr ||
      (g8 == nullptr) != (gt8 == nullptr) || (mode != 0 && mode != 1))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)img_ids | (uintptr_t)txt_ids) % 8 != 0 ||
      ((uintptr_t)tprime | (uintptr_t)bias | (uintptr_t)ws) % 4 != 0)
    return (int)hipErrorInvalidValue;
  if (g8 != nullptr && (ldg < n || ldgt < b)) return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if (!pair_grid_ok(tiles_m, tiles_n)) return (int)hipErrorInvalidValue;
  const auto kernel = g8 != nullptr ? sigmoid_ids_mx_kernel<true>
                                    : sigmoid_ids_mx_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(tiles_m * tiles_n), dim3(NTHREADS), 0,
                     (hipStream_t)stream, (const unsigned char*)zimg_q,
                     (const unsigned char*)zimg_e8,
                     (const unsigned char*)ztxt_q,
                     (const unsigned char*)ztxt_e8, (const float*)tprime,
                     (const float*)bias, (const long long*)img_ids,
                     (const long long*)txt_ids, (unsigned char*)g8,
                     (unsigned char*)gt8, (float*)ws, b, n, d, (int)lde_img,
                     ldg, ldgt, diag, mode, tiles_m, tiles_n);
  return (int)hipGetLastError();
}

}  // extern "C"
