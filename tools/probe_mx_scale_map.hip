// probe_mx_scale_map.hip — which (lane, byte) of the two scale operands does
// v_mfma_scale_f32_16x16x128_f8f6f4 (gfx950) apply to which row and which k?
//
// One wave.  A is all 1.0 and B holds 2^g in all 32 bytes of lane group
// g = lane >> 4, so an output is 32·(1 + 2 + 4 + 8) = 480 with unit scales.
// Per MFMA one byte of one lane's scale dword is raised by 2^10, for every
// lane, byte, op_sel value and both operands; the host prints, for each MFMA
// that changed anything, how many outputs moved, the first one's (row, col)
// and log2 of the scaled share of the sum in units of 32: 0.58 = log2(1.5) is
// half of groups 0 and 1, 2.58 = log2(6) half of groups 2 and 3.  Result
// (profiles/mx_scale_map.log): only byte op_sel is read; lane l scales row
// (column) l & 15; lane group kb scales hardware k 32·kb … +31, where lane l's
// registers 0–3 are k 16·(l >> 4) … +15 and 4–7 are 64 + 16·(l >> 4) … +15.
// pair_tile.h's MX main loop is built on this.
//
// Build+run (GPU box):
//   hipcc --offload-arch=gfx950 -O2 tools/probe_mx_scale_map.hip -o /tmp/mxm && /tmp/mxm
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
#define CHK(x) do { hipError_t e = (x); if (e) { printf("HIP error %d at %d\n", (int)e, __LINE__); exit(1); } } while (0)

template <int OPSEL>
__device__ void sweep(float* out /* [2][64][4][256] */) {
  const int lane = threadIdx.x & 63;
  const int kb = lane >> 4;
  const unsigned bcode = 0x38u + 8u * kb;           // 2^kb
  i32x8 a, b;
  for (int i = 0; i < 8; ++i) { a[i] = 0x38383838; b[i] = (int)(bcode * 0x01010101u); }
  for (int side = 0; side < 2; ++side)
    for (int L = 0; L < 64; ++L)
      for (int byte = 0; byte < 4; ++byte) {
        unsigned s = 0x7f7f7f7fu;
        if (lane == L) s = (s & ~(0xffu << (8 * byte))) | (137u << (8 * byte));
        const unsigned sa = side == 0 ? s : 0x7f7f7f7fu;
        const unsigned sb = side == 1 ? s : 0x7f7f7f7fu;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, OPSEL, (int)sa, OPSEL, (int)sb);
        float* o = out + (((long)side * 64 + L) * 4 + byte) * 256;
        for (int r = 0; r < 4; ++r) o[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
      }
}
__global__ void k(float* out) {
  sweep<0>(out);
  sweep<1>(out + 2 * 64 * 4 * 256);
  sweep<2>(out + 2 * 2 * 64 * 4 * 256);
  sweep<3>(out + 3 * 2 * 64 * 4 * 256);
}
int main() {
  const size_t n = 4ul * 2 * 64 * 4 * 256;
  float* d; CHK(hipMalloc(&d, n * 4));
  hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d);
  CHK(hipDeviceSynchronize());
  std::vector<float> h(n); CHK(hipMemcpy(h.data(), d, n * 4, hipMemcpyDeviceToHost));
  for (int op = 0; op < 4; ++op) for (int side = 0; side < 2; ++side) for (int L = 0; L < 64; ++L) for (int byte = 0; byte < 4; ++byte) {
    const float* o = &h[((((size_t)op * 2 + side) * 64 + L) * 4 + byte) * 256];
    int cnt = 0, r0 = -1, c0 = -1; float v = 0;
    for (int i = 0; i < 256; ++i) if (o[i] != 480.f) { if (!cnt) { r0 = i / 16; c0 = i % 16; v = o[i]; } ++cnt; }
    if (cnt) {
      // v = 480 + 32*2^kb*1023
      const double kbf = log2((v - 480.0) / (32.0 * 1023.0));
      printf("opsel%d side%c lane%2d byte%d -> %3d changed, first (row %2d, col %2d) kblock %.2f\n", op, side ? 'B' : 'A', L, byte, cnt, r0, c0, kbf);
    }
  }
  printf("base %.1f\n", h[0]);
  return 0;
}
