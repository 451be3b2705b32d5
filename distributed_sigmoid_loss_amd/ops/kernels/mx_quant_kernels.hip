// MXFP8 quantiser for gfx950 (MI355X): bf16 (rows, d), d % 32 == 0, to OCP
// e4m3fn elements with one e8m0 scale per block of 32 consecutive elements —
// the operand format of v_mfma_scale_f32_16x16x128_f8f6f4 as pair_tile.h's MX
// main loop feeds it.  One pass, no atomics, no host sync.
//
//   q  (rows, d) bytes         x ≈ q·2^(code − 127), block by block
//   e8 (rows, w) bytes, w = 4·ceil(d / 128): byte kb of a row is the code of
//      elements 32·kb … 32·kb + 31; bytes past d / 32 are 0x7F.  A row is a
//      whole number of aligned dwords, one per 128-element K-step.
//
// Rule.  amax = m·2^p, m in [1, 2): e = p − 8 if m ≤ 1.75, else p − 7 — the
// smallest power of two with amax·2^−e ≤ 448, so nothing saturates — clamped
// to [−127, 127]; code = e + 127; an all-zero block gets 0x7F.  Elements are
// x·2^−e (exact in fp32) rounded to nearest even by v_cvt_pk_fp8_f32.  All of
// it from the bits: |bf16| orders as a 15-bit integer, so amax is an integer
// max, p + 127 its exponent field E and m ≤ 1.75 its mantissa field ≤ 0x60:
//   code = max(E − 8 + (mantissa > 0x60), 0)
// (a denormal amax has E = 0 and clamps like the smallest normals), and
// 2^−e is the float with exponent field 254 − code.  Non-finite input is
// unspecified.
//
// Work split.  A block is 64 bytes of bf16 and one lane owns it: four 16-byte
// loads, an integer max over the 32 halves, 16 conversions, two 16-byte
// stores.  Lanes are laid over the (rows, w) grid of scale bytes, pad bytes
// included, so the four lanes of a DPP quad hold the four bytes of one scale
// dword: two quad-permute moves assemble it and lane 0 of the quad writes it —
// every byte of e8 is written, none read.  With d = 768 (w = 24) no lane
// idles.  Bounded grid, grid-stride over the scale bytes; the (row, block) of
// a lane is advanced by the stride's quotient and remainder, one division at
// the start.

#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

constexpr int QT = 256;            // threads per workgroup
constexpr int MAX_BLOCKS = 512;    // two per CU

__launch_bounds__(QT) __global__ void quant_mx_bf16_kernel(
    const unsigned short* __restrict__ x, unsigned char* __restrict__ q,
    unsigned* __restrict__ e8, int d, int w, long long slots, int step_rows,
    int step_kb) {
  const int nblk = d >> 5;
  const int lane = threadIdx.x & 63;
  const unsigned first = blockIdx.x * QT + threadIdx.x;
  long long slot = first;
  long long row = first / (unsigned)w;
  int kb = (int)(first % (unsigned)w);
  const long long stride = (long long)gridDim.x * QT;

  // `slots` is a multiple of 4 and a quad starts at one: a quad is inside or
  // outside as a whole, and the loop is left by whole waves only.
  for (; slot - lane < slots; slot += stride) {
    const bool inside = slot < slots;
    unsigned code = 0x7F;
    if (inside && kb < nblk) {
      const long long at = row * d + 32 * kb;
      uint4 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = reinterpret_cast<const uint4*>(x + at)[i];
      const unsigned* u = reinterpret_cast<const unsigned*>(v);
      unsigned lo = 0, hi = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const unsigned a = u[i] & 0x7FFF7FFFu;
        lo = max(lo, a & 0xFFFFu);
        hi = max(hi, a >> 16);
      }
      const int amax = (int)max(lo, hi);
      if (amax != 0)
        code = (unsigned)max((amax >> 7) - 8 + ((amax & 0x7F) > 0x60), 0);
      const float r = __uint_as_float((254u - code) << 23);      // 2^−e
      unsigned out[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const unsigned p0 = u[2 * i], p1 = u[2 * i + 1];
        int c = __builtin_amdgcn_cvt_pk_fp8_f32(
            __uint_as_float(p0 << 16) * r,
            __uint_as_float(p0 & 0xFFFF0000u) * r, 0, false);
        c = __builtin_amdgcn_cvt_pk_fp8_f32(
            __uint_as_float(p1 << 16) * r,
            __uint_as_float(p1 & 0xFFFF0000u) * r, c, true);
        out[i] = (unsigned)c;
      }
      uint4* dst = reinterpret_cast<uint4*>(q + at);
      dst[0] = uint4{out[0], out[1], out[2], out[3]};
      dst[1] = uint4{out[4], out[5], out[6], out[7]};
    }
    // The quad's four codes as one dword, byte = lane & 3.
    unsigned word = code << (8 * (lane & 3));
    word |= (unsigned)__builtin_amdgcn_mov_dpp((int)word, 0xB1, 0xf, 0xf, true);
    word |= (unsigned)__builtin_amdgcn_mov_dpp((int)word, 0x4E, 0xf, 0xf, true);
    if (inside && (lane & 3) == 0) e8[slot >> 2] = word;

    row += step_rows;
    kb += step_kb;
    if (kb >= w) {
      kb -= w;
      ++row;
    }
  }
}

}  // namespace

extern "C" {

// x: bf16 (rows, d) row-major contiguous, d a positive multiple of 32;
// q: (rows, d) bytes; e8: (rows, 4·ceil(d / 128)) bytes, all of them written.
// x and q 16-byte aligned, e8 4-byte aligned.  Returns non-zero, launching
// nothing, on anything unsupported.
int quant_mx_bf16(uintptr_t stream, const void* x, void* q, void* e8,
                  int rows, int d) {
  if (x == nullptr || q == nullptr || e8 == nullptr || rows < 1 || d < 32 ||
      d % 32 != 0)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)q) % 16 != 0 || (uintptr_t)e8 % 4 != 0)
    return (int)hipErrorInvalidValue;
  const int w = 4 * ((d + 127) / 128);
  const long long slots = (long long)rows * w;
  const long long want = (slots + QT - 1) / QT;
  const int blocks = want < MAX_BLOCKS ? (int)want : MAX_BLOCKS;
  const int stride = blocks * QT;
  hipLaunchKernelGGL(quant_mx_bf16_kernel, dim3(blocks), dim3(QT), 0,
                     (hipStream_t)stream, (const unsigned short*)x,
                     (unsigned char*)q, (unsigned*)e8, d, w, slots,
                     stride / w, stride % w);
  return (int)hipGetLastError();
}

}  // extern "C"
