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
// Structure (the softmax kernel's tile).  128×128 output tile per 256-thread
// workgroup, 4 waves as 2 (M) × 2 (N), 64×64 (4×4 fragments of
// v_mfma_f32_16x16x32_bf16) each, fp32 accumulation.  A k-step stages a
// [128 rows][64 k] slab of each operand in LDS (double-buffered, 2 × 32 KiB)
// through registers with 16-byte loads; rows past b / n and k past d are
// zero-filled.  The 16-byte chunk index is XOR-ed with (row >> 1) & 7.  The
// MFMA operands are exchanged (text fragment first): lane l owns image row
// (l & 15) and the four consecutive text columns 4·(l >> 4) … +3 of each
// fragment.  Two workgroups (64 KiB each) share a CU.
//
// Ids.  Once the K loop's last barrier has passed, the tile's 128 row ids and
// 128 column ids are staged as int64 in the 2 KiB above the g staging area;
// a row or column outside the block gets id −1 there, so padding is masked by
// the same test as a negative id.  The mask matters: a zero-filled padding
// element has z = bias, not 0, and would add softplus(bias) to the loss.  The
// epilogue walks the fragments column-major, so a lane keeps its 4 row ids
// in registers and reads the 4 column ids of one fragment at a time.
//
// exp / log are the bare v_exp_f32 / v_log_f32 (base 2) with the ln 2 factors
// folded in; 1 / (1 + e) is v_rcp_f32 (1 ulp, 2⁻¹⁶ of a bf16 ulp).
//
// Placement.  One workgroup per tile on a 1-D grid; the block id is remapped
// so consecutive logical ids share an XCD, and logical ids walk the tile grid
// in groups of 8 tile-rows, column by column.

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
constexpr int IDS_OFF = G_STAGE_BYTES;        // 128 row ids, 128 column ids
constexpr int IDS_BYTES = (BM + BN) * 8;      // 2 KiB
constexpr int RED_OFF = IDS_OFF + IDS_BYTES;  // 4 waves × 3 partials
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

static_assert(IDS_OFF % 16 == 0, "id staging must take 16-byte reads");
static_assert(RED_OFF + 64 <= 2 * BUF_BYTES, "epilogue staging exceeds LDS");

inline int ceil_div(int a, int b) { return (a - 1) / b + 1; }  // a ≥ 1

// Byte offset of 16-byte chunk `ch` (0..7) of row `row` in an operand slab.
__device__ __forceinline__ int lds_off(int row, int ch) {
  return ROW_BYTES * row + 16 * (ch ^ ((row >> 1) & 7));
}

struct TilePos { int tm, tn; };

// XCD-contiguous (bijective) remap, then the grouped column-major walk.
__device__ __forceinline__ TilePos tile_of_block(int tiles_m, int tiles_n) {
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
  return TilePos{first_m + in_group % group_h, in_group / group_h};
}

// acc[i][j][r] = <zimg row m0 + wm·64 + i·16 + (lane & 15),
//                 ztxt row n0 + wn·64 + j·16 + 4·(lane >> 4) + r>
// (0 where either row lies outside its matrix).  Ends on a barrier: every
// read of the staging buffers has retired, the caller may reuse `lds`.
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
      // Text fragment first: the accumulator is the transposed block.
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              bfr[j], af[i], acc[i][j], 0, 0, 0);
    }

    if (more) store_step((s + 1) & 1);
    __syncthreads();
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

  const TilePos tp = tile_of_block(tiles_m, tiles_n);
  const int m0 = tp.tm * BM, n0 = tp.tn * BN;
  f32x4 acc[4][4];
  pair_tile_dots(zimg, ztxt, b, n, d, m0, n0, lds, acc);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const float t = expf(tprime[0]);
  const float bs = bias[0];
  const bool ignore = ignore_dups != 0;

  // Stage the tile's ids: threads 0..127 a row id, 128..255 a column id;
  // −1 outside the block.
  long long* idl = reinterpret_cast<long long*>(lds + IDS_OFF);
  {
    const bool is_row = tid < BM;
    const int e = is_row ? m0 + tid : n0 + (tid - BM);
    const int len = is_row ? b : n;
    const long long* src = is_row ? img_ids : txt_ids;
    long long id = -1;
    if (e < len) id = src[e];
    idl[tid] = id;
  }
  __syncthreads();

  // This lane's four rows: id, and the column of the row's positional
  // positive ("ignore" only; −1 when it has none inside the block).
  long long rid[4];
  int pc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lrow = wm * 64 + i * 16 + fr;
    rid[i] = idl[lrow];
    const long long pos = (long long)(m0 + lrow) + diag;
    pc[i] = (ignore && diag != DIAG_NONE && pos >= 0 && pos < n) ? (int)pos
                                                                 : -1;
  }

  float s_loss = 0.f, s_gs = 0.f, s_g = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int lcol0 = wn * 64 + j * 16 + fq * 4;
    const int col0 = n0 + lcol0;
    long long cid[4];
    {
      const longlong2 c01 =
          *reinterpret_cast<const longlong2*>(idl + BM + lcol0);
      const longlong2 c23 =
          *reinterpret_cast<const longlong2*>(idl + BM + lcol0 + 2);
      cid[0] = c01.x; cid[1] = c01.y; cid[2] = c23.x; cid[3] = c23.y;
    }
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

  // Write-out: 16 threads cover one 256-byte tile row.  A 16-byte store
  // where the segment is whole and its address aligned, 2-byte stores
  // otherwise (ragged edge, odd row stride or column offset).
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
  if (zimg == nullptr || ztxt == nullptr || tprime == nullptr ||
      bias == nullptr || img_ids == nullptr || txt_ids == nullptr ||
      ws == nullptr)
    return (int)hipErrorInvalidValue;
  if (b < 1 || n < 1 || d < 8 || d % 8 != 0 || (mode != 0 && mode != 1))
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)zimg | (uintptr_t)ztxt) % 16 != 0 ||
      ((uintptr_t)img_ids | (uintptr_t)txt_ids) % 8 != 0 ||
      ((uintptr_t)tprime | (uintptr_t)bias | (uintptr_t)ws) % 4 != 0 ||
      (uintptr_t)g % 2 != 0)
    return (int)hipErrorInvalidValue;
  if (g != nullptr && ldg < n) return (int)hipErrorInvalidValue;
  const int tiles_m = ceil_div(b, BM), tiles_n = ceil_div(n, BN);
  if ((long long)tiles_m * tiles_n >= (1ll << 31))
    return (int)hipErrorInvalidValue;
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
