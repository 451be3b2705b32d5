// Split-K weight-gradient GEMM and in-place bf16 scale for gfx950 (MI355X).
//
//   dW[M,N] = Aᵀ·X     A (K, M) and X (K, N) bf16 row-major (unit column
//                      stride, row strides lda / ldx), dW bf16, fp32
//                      accumulation on v_mfma_f32_16x16x32_bf16.
//
// This is the projection towers' weight gradient: A = dY, X = the tower
// input, K = the batch.  The output is small (768×768 at the flagship shape)
// and K is huge (32768), so a plain output-tiled GEMM occupies 24–36 CUs.
// Here the grid is (output tiles) × (K slices), sized to about twice the CU
// count (two workgroups fit on a CU).
//
// Operand staging.  Both operands are batch-strided: memory is contiguous
// along M / N while the MFMA wants 8 consecutive k per lane.  Each k-step
// stages a row-major [BK][128] slab of each operand in LDS with coalesced
// 16-byte loads (register staging, so rows past the slice end and columns
// past M / N are zero-filled rather than masked) and forms the K-major
// fragments with ds_read_b64_tr_b16, the 4×16 hardware transpose read.  The
// A and X fragments of a lane take the same k for the same element index, so
// the k order inside a fragment is free; lane l>>4 = g takes k rows
// 8g … 8g+7 of each 32-deep MFMA step in two 4-row reads.  The LDS image is
// plain 256-byte rows with the 16-byte chunk index XOR-ed by
// ((row&3)<<2 | (row>>2)&3), which keeps both the ds_write_b128 fill and the
// transposed reads (two 4-row blocks 8 rows apart per 32-lane half) off
// each other's banks.
//
// Reduction.  Slices write fp32 partial tiles to a caller-provided workspace
// [slices][M][N]; a second kernel sums them in slice order and rounds once to
// bf16.  No atomics, no arrival counters: the result is bitwise reproducible.
// Empty slices (fewer k-steps than slices) write zeros.
//
// Placement.  Workgroups are dispatched round-robin over the 8 XCDs; the
// block id is remapped so consecutive logical ids share an XCD, and logical
// id = slice·tiles + tile, so the tiles of one K slice run together on one
// XCD and each slab is fetched into that XCD's L2 once.

#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

constexpr int BM = 128;          // output tile rows   (columns of A)
constexpr int BN = 128;          // output tile cols   (columns of X)
constexpr int BK = 64;           // batch rows per k-step
constexpr int NTHREADS = 256;    // 4 waves as 2 (M) × 2 (N), 64×64 each
constexpr int ROW_BYTES = 256;   // one 128-column bf16 LDS row
constexpr int OP_BYTES = BK * ROW_BYTES;      // one operand slab: 16 KiB
constexpr int BUF_BYTES = 2 * OP_BYTES;       // A slab + X slab
constexpr int LOADS = BK * 16 / NTHREADS;     // 16-B chunks per thread: 4
constexpr int MAX_SLICES = 64;

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// Byte offset of 16-byte chunk `ch` (0..15) of row `row` in an operand slab.
__device__ __forceinline__ int lds_off(int row, int ch) {
  return ROW_BYTES * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

// Round-to-nearest-even fp32 → bf16 bits (NaN → quiet NaN), as torch does.
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

__device__ __forceinline__ float bf16_bits_to_f32(unsigned short h) {
  return __uint_as_float((unsigned)h << 16);
}

__launch_bounds__(NTHREADS) __global__ void wgrad_splitk_kernel(
    const __bf16* __restrict__ A, const __bf16* __restrict__ X,
    float* __restrict__ ws, int K, int M, int N, long long lda,
    long long ldx, int slices, int tiles_n, int tiles, int grid_per_xcd) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUF_BYTES];

  // XCD-contiguous remap, then logical id = slice * tiles + tile.
  const int lid = (int)(blockIdx.x & 7) * grid_per_xcd + (int)(blockIdx.x >> 3);
  if (lid >= tiles * slices) return;
  const int slice = lid / tiles;
  const int tile = lid - slice * tiles;
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;

  const int ksteps = ceil_div(K, BK);
  const int per = ceil_div(ksteps, slices);
  const int s_begin = slice * per;
  const int s_end = (s_begin + per < ksteps) ? s_begin + per : ksteps;
  const int nsteps = s_end > s_begin ? s_end - s_begin : 0;
  const int k_end = (s_end * BK < K) ? s_end * BK : K;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // Staging: thread t owns chunk t&15 of rows (t>>4) + 16·i, i = 0..3.
  const int ld_ch = tid & 15;
  const int ld_row = tid >> 4;
  const bool a_col_ok = m0 + ld_ch * 8 < M;
  const bool x_col_ok = n0 + ld_ch * 8 < N;
  const __bf16* a_src = A + m0 + ld_ch * 8;
  const __bf16* x_src = X + n0 + ld_ch * 8;
  int st_off[LOADS];
#pragma unroll
  for (int i = 0; i < LOADS; ++i) st_off[i] = lds_off(ld_row + 16 * i, ld_ch);

  // Transposed-read addresses.  Lane 4q+p of a 16-lane group supplies row
  // r0+q, elements 4p … 4p+3 of the 16-column block; group g reads rows
  // 8g + 4h + (0..3) of each 32-row MFMA step (h = 0, 1).
  const int grp = lane >> 4;
  const int q = (lane >> 2) & 3, p = lane & 3;
  int a_off[4][2], x_off[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 8 * grp + 4 * h + q;
      a_off[f][h] = lds_off(row, wm * 8 + f * 2 + (p >> 1)) + 8 * (p & 1);
      x_off[f][h] = OP_BYTES + lds_off(row, wn * 8 + f * 2 + (p >> 1))
                    + 8 * (p & 1);
    }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 ra[LOADS], rx[LOADS];

  auto load_step = [&](int s) {
    const int k0 = s * BK + ld_row;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int k = k0 + 16 * i;
      ra[i] = uint4{0u, 0u, 0u, 0u};
      rx[i] = uint4{0u, 0u, 0u, 0u};
      if (k < k_end) {
        if (a_col_ok)
          ra[i] = *reinterpret_cast<const uint4*>(a_src + (long long)k * lda);
        if (x_col_ok)
          rx[i] = *reinterpret_cast<const uint4*>(x_src + (long long)k * ldx);
      }
    }
  };
  auto store_step = [&](int buf) {
    unsigned char* base = lds + buf * BUF_BYTES;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      *reinterpret_cast<uint4*>(base + st_off[i]) = ra[i];
      *reinterpret_cast<uint4*>(base + OP_BYTES + st_off[i]) = rx[i];
    }
  };

  if (nsteps > 0) {
    load_step(s_begin);
    store_step(0);
  }
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;
    if (more) load_step(s_begin + s + 1);

    const lds_bf16x4* base = (const lds_bf16x4*)(lds + (s & 1) * BUF_BYTES);
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8 af[4], xf[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int ko = kk * 32 * ROW_BYTES;
        const bf16x4 a_lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (lds_bf16x4*)((const __attribute__((address_space(3)))
                           unsigned char*)base + a_off[f][0] + ko));
        const bf16x4 a_hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (lds_bf16x4*)((const __attribute__((address_space(3)))
                           unsigned char*)base + a_off[f][1] + ko));
        const bf16x4 x_lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (lds_bf16x4*)((const __attribute__((address_space(3)))
                           unsigned char*)base + x_off[f][0] + ko));
        const bf16x4 x_hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (lds_bf16x4*)((const __attribute__((address_space(3)))
                           unsigned char*)base + x_off[f][1] + ko));
        af[f] = __builtin_shufflevector(a_lo, a_hi, 0, 1, 2, 3, 4, 5, 6, 7);
        xf[f] = __builtin_shufflevector(x_lo, x_hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[i], xf[j], acc[i][j], 0, 0, 0);
    }

    if (more) store_step((s + 1) & 1);
    __syncthreads();
  }

  // fp32 partial tile → workspace[slice][M][N].  C layout of the 16×16 MFMA:
  // col = lane & 15, row = (lane >> 4) * 4 + reg.
  float* out = ws + (size_t)slice * M * N;
  const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 64 + i * 16 + fq * 4 + r;
        if (m < M && n < N) out[(size_t)m * N + n] = acc[i][j][r];
      }
    }
}

// Sum the slices' partials in slice order, round once to bf16.  One thread
// per 4 consecutive outputs (M·N is a multiple of 4 since N % 8 == 0).
__launch_bounds__(256) __global__ void wgrad_reduce_kernel(
    const float* __restrict__ ws, unsigned short* __restrict__ dw,
    int total4, int slices) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const float4* src = reinterpret_cast<const float4*>(ws) + i;
  float4 s = src[0];
  for (int k = 1; k < slices; ++k) {
    const float4 v = src[(size_t)k * total4];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  ushort4 o;
  o.x = f32_to_bf16_bits(s.x);
  o.y = f32_to_bf16_bits(s.y);
  o.z = f32_to_bf16_bits(s.z);
  o.w = f32_to_bf16_bits(s.w);
  reinterpret_cast<ushort4*>(dw)[i] = o;
}

// x[i] = bf16(float(x[i]) · float(bf16(*scale))) in place: 16-byte accesses,
// grid-stride loop, scalar tail.  Matches torch's bf16 tensor × bf16 0-d
// tensor (fp32 product, one round-to-nearest-even).
__launch_bounds__(256) __global__ void scale_bf16_inplace_kernel(
    unsigned short* __restrict__ x, const float* __restrict__ scale,
    long long n) {
  const float s = bf16_bits_to_f32(f32_to_bf16_bits(*scale));
  const long long n8 = n >> 3;
  const long long stride = (long long)gridDim.x * 256;
  uint4* x8 = reinterpret_cast<uint4*>(x);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8;
       i += stride) {
    uint4 v = x8[i];
    unsigned* w = reinterpret_cast<unsigned*>(&v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned lo = f32_to_bf16_bits(
          bf16_bits_to_f32((unsigned short)(w[k] & 0xffffu)) * s);
      const unsigned hi = f32_to_bf16_bits(
          bf16_bits_to_f32((unsigned short)(w[k] >> 16)) * s);
      w[k] = lo | (hi << 16);
    }
    x8[i] = v;
  }
  for (long long i = (n8 << 3) + (long long)blockIdx.x * 256 + threadIdx.x;
       i < n; i += stride)
    x[i] = f32_to_bf16_bits(bf16_bits_to_f32(x[i]) * s);
}

bool wgrad_dims_ok(int K, int M, int N) {
  return K > 0 && M > 0 && N > 0 && M % 8 == 0 && N % 8 == 0;
}

}  // namespace

extern "C" {

// Number of K slices for a (K, M, N) problem on a device with `n_cu` compute
// units: tiles × slices ≈ 2·n_cu — two workgroups (64 KiB LDS, 188 VGPRs
// each) are co-resident per CU and hide each other's staging latency; the
// sweep in profiles/wgrad_sweep.log has 14 slices (504 workgroups on 256
// CUs) fastest at the flagship shape, and a count just past 2·n_cu (16
// slices) paying a second wave of workgroups.  At least two k-steps per
// slice, at most MAX_SLICES.  Returns 0 for unsupported dims.
int linear_wgrad_plan(int K, int M, int N, int n_cu) {
  if (!wgrad_dims_ok(K, M, N) || n_cu <= 0) return 0;
  const int tiles = ceil_div(M, BM) * ceil_div(N, BN);
  const int ksteps = ceil_div(K, BK);
  int s = 2 * n_cu / tiles;
  if (s > ksteps / 2) s = ksteps / 2;
  if (s > MAX_SLICES) s = MAX_SLICES;
  return s < 1 ? 1 : s;
}

// dW (M, N) bf16 = Aᵀ·X with A (K, M), X (K, N) bf16, row strides lda / ldx
// elements.  `ws` holds slices·M·N floats.  Returns non-zero, launching
// nothing, on anything unsupported: null pointers, M or N not a multiple of
// 8, operands or strides that break the 16-byte loads, a bad slice count.
int linear_wgrad_bf16(uintptr_t stream, const void* a, const void* x,
                      void* ws, void* dw, int K, int M, int N, long long lda,
                      long long ldx, int slices) {
  if (a == nullptr || x == nullptr || ws == nullptr || dw == nullptr)
    return (int)hipErrorInvalidValue;
  if (!wgrad_dims_ok(K, M, N) || slices < 1 || slices > MAX_SLICES)
    return (int)hipErrorInvalidValue;
  if (lda < M || ldx < N || lda % 8 != 0 || ldx % 8 != 0)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)a | (uintptr_t)x | (uintptr_t)ws) % 16 != 0 ||
      (uintptr_t)dw % 8 != 0)
    return (int)hipErrorInvalidValue;
  if ((long long)M * N >= (1ll << 31)) return (int)hipErrorInvalidValue;
  const int tiles_n = ceil_div(N, BN);
  const int tiles = ceil_div(M, BM) * tiles_n;
  const int grid_per_xcd = ceil_div(tiles * slices, 8);
  hipLaunchKernelGGL(wgrad_splitk_kernel, dim3(grid_per_xcd * 8),
                     dim3(NTHREADS), 0, (hipStream_t)stream,
                     (const __bf16*)a, (const __bf16*)x, (float*)ws, K, M, N,
                     lda, ldx, slices, tiles_n, tiles, grid_per_xcd);
  const int total4 = M * N / 4;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(ceil_div(total4, 256)),
                     dim3(256), 0, (hipStream_t)stream, (const float*)ws,
                     (unsigned short*)dw, total4, slices);
  return (int)hipGetLastError();
}

// In-place x *= bf16(*scale) on a contiguous bf16 tensor of n elements;
// `scale` is a device fp32 scalar.
int scale_bf16_inplace(uintptr_t stream, void* x, const void* scale,
                       long long n) {
  if (x == nullptr || scale == nullptr || n < 0 || (uintptr_t)x % 16 != 0 ||
      (uintptr_t)scale % 4 != 0)
    return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  long long blocks = ((n >> 3) + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_bf16_inplace_kernel, dim3((int)blocks), dim3(256),
                     0, (hipStream_t)stream, (unsigned short*)x,
                     (const float*)scale, n);
  return (int)hipGetLastError();
}

}  // extern "C"
