// siglip_kernels.hip — fused SigLIP sigmoid-loss kernels for MI355X (gfx950, CDNA4).
//
// Implements, per (b, n) block of image×text embeddings (row-major, K = emb
// dim contiguous; bf16 or OCP fp8-e4m3):
//
//   forward:  loss += sum_ij softplus(-l_ij * (t * <zimg_i, ztxt_j> + bias))
//   backward: g_ij  = -l_ij * sigmoid(-l_ij * z_ij)   (slab: bf16, or e4m3
//             ×448 plus its transpose for the fp8/mixed grad-GEMM policies)
//             scal[0] += sum g_ij * <zimg_i, ztxt_j>   (for dt')
//             scal[1] += sum g_ij                      (for dbias)
//
// with labels l_ij = +1 iff j == i + diag_offset (an index predicate — the
// (b,n) label matrix of the reference, distributed_sigmoid_loss.py:28-30 and
// rwightman_sigmoid_loss.py:43-47, is never materialized), l_ij = -1 else.
// The (b,n) logits matrix never leaves the MFMA accumulators; only the g
// slab consumed by the two library GEMMs (dzimg = t·g@ztxt,
// dztxt = t·gᵀ@zimg, ops/__init__.py) ever reaches memory.
//
// MODE 2 ("fwd+g") fuses the two: one kernel emits the loss, the g slab and
// both scalar partials, so a training step never computes the logits GEMM
// twice — backward is then pure GEMMs on the saved slab (the reference's
// autograd does exactly this by saving the logits graph; here the saved
// state is the (b,n) g slab, e.g. 2 GiB at B=32k bf16, trivial against
// 288 GB HBM3E).  The recompute MODE 1 remains for the huge-batch chunked
// path where the slab would not fit (BASELINE config 3).
//
// Kernel structure (templates: MODE 0 = fwd, 1 = bwd-g, 2 = fwd+g; EB = element bytes,
// 2 = bf16 via v_mfma_f32_16x16x32_bf16, 1 = fp8-e4m3 via the MX-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales — 2× the bf16
// MFMA rate and half the staged bytes; per-tensor scales are folded into the
// temperature by the Python wrapper):
//   - 256×256 output tile per 512-thread (8-wave, 2×4) workgroup; each wave
//     owns a 128×64 sub-tile as 8×4 fragments, fp32 accumulate.
//   - K-loop in 128-byte K-steps (64 bf16 / 128 fp8 elements), double-
//     buffered LDS (4×32 KiB) staged by global_load_lds_dwordx4 (direct
//     HBM→LDS DMA).  The LDS image is [K-half][row][64 B]: bf16 stages and
//     waits at K-HALF granularity interleaved with the two MFMA half-steps,
//     so every 16 KiB granule gets a full iteration of transfer window.
//     (Measured limit at B≥16k: the DMA+MFMA co-run itself — staging alone
//     0.469 ms, compute alone 0.449, decoupled co-run 0.598, full 0.632 —
//     finer schedules up to a complete 8-phase fragment-unit pipeline
//     [tools/probe_8phase.hip] are neutral; see profiles/README.md.)
//   - The DMA stays in flight across raw s_barriers under counted
//     s_waitcnt vmcnt(N) (a __syncthreads would drain it); barriers are
//     asm statements with "memory" clobbers — the plain s_barrier builtin
//     is not a compiler fence and ds_reads were observed hoisted above it.
//   - Bank swizzle on the 16-B chunk index (both-sides rule, source address
//     + ds_read offset): chunk' = chunk ^ ((row>>2)&3) within each 64-B
//     half-row — conflict-free b128 fragment reads under both contiguous
//     and interleaved lane grouping.
//   - All addressing is precomputed per lane (recomputing it per tile
//     measured VALU-bound: VALUBusy ≈ 5×MfmaUtil); the K advance rides the
//     uniform base pointers (SALU), the buffer toggle is one XOR.
//   - Edge blocks (ragged b/n, short d) take a register-staged path writing
//     the same LDS image with zero-fill guards; the interior kernel is
//     compiled separately so the hot path's register allocation is not
//     inflated by the guarded path (spill-free).
//   - Block-id remap (flags): bit0 = XCD-contiguous spans, bit1 = grouped
//     column-major walk — temporally-close blocks share operand panels in
//     the per-XCD L2 (measured best together: +4%).
//   - Epilogue (all modes and dtypes): exp2 and log2 are the bare
//     v_exp_f32 / v_log_f32 (the log argument 1+y stays in (1,2]; the log2
//     sum meets ln 2 once per tile); the label predicate is block-uniform —
//     a tile that cannot hold a positive pair runs a body without it in the
//     interior kernels, the rest compare one per-lane constant; where the
//     bf16 g slab stages through LDS the MFMA operands are exchanged so a
//     lane packs 4 consecutive g columns into one ds_write_b64.
//   - bf16 interior shapes run a PERSISTENT kernel
//     (siglip_tile_kernel_persistent): min(tiles, CUs) workgroups walk the
//     tile list with one K-stream across tile boundaries, per-wave g
//     staging above the operand buffers (no block barrier in the epilogue)
//     and one scalar reduction + three atomics per workgroup.  The e4m3-g
//     instantiations (g + gᵀ staging needs all of LDS) and the edge kernel
//     stay one tile per workgroup.
//
// Host interface: every instantiation of the tile kernel is reached through
// ONE exported function of fixed signature, siglip_tile(stream, mode, eb,
// eb_g, ...), which validates its arguments and switches to launch<>; the
// Python side (ops/__init__.py::_launch_tile) is its only caller.  The
// l2norm_* and quant_fp8_* helpers keep one small export each.
//
// Requirements: bf16 d%8==0, fp8 d%16==0; b, n arbitrary (guarded path).
// Compile: hipcc --offload-arch=gfx950 -O3 -shared -fPIC.

#include <hip/hip_runtime.h>
#include <hip/hip_fp8.h>
#include <cstdint>
#include <climits>
#include <type_traits>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef const __attribute__((address_space(1))) unsigned int* gas_ptr;
typedef __attribute__((address_space(3))) unsigned int* las_ptr;

namespace {

constexpr int BM = 256;          // image rows per block
constexpr int BN = 256;          // text rows (logit cols) per block
constexpr int THREADS = 512;     // 8 waves as 2(M)×4(N)
constexpr int FM = 8;            // M fragments per wave (128 rows)
constexpr int FN = 4;            // N fragments per wave (64 cols)
constexpr int HROW = 64;         // bytes per row within one K-half
constexpr int HALF_BYTES = BM * HROW;        // 16 KiB per operand K-half
constexpr int TILE_BYTES = 2 * HALF_BYTES;   // 32 KiB per operand K-step
constexpr int DIAG_NONE = INT_MIN;
constexpr int NXCD = 8;
constexpr int OUT_STRIDE = 32;   // floats per XCD slot of the scalar-output
                                 // buffer (128 B = one cache line)
constexpr int GROUP_M = 8;       // block-rows per locality group (bit1)

// softplus(x) = max(x,0) + log(1+y), y = e^{-|x|} ∈ (0,1].  The log argument
// never leaves (1, 2], so the bare v_log_f32 (log2, ~1 ulp) needs none of
// __logf's denormal pre-scale / compensated ln2 multiply / range guards
// (about eleven VALU per element in the ISA; log1pf is a device-lib CALL).
// The two parts go to separate per-lane sums: the log2 sum is multiplied by
// ln 2 ONCE per tile when it is folded into the loss partial.  The naive
// 1+y loses only ~y·ε absolute accuracy near y→0, where the term vanishes.
constexpr float LN2_F = 0.693147180559945309f;
__device__ __forceinline__ void softplus_acc(float x, float y, float& s_relu,
                                             float& s_log2) {
  s_relu += fmaxf(x, 0.0f);
  s_log2 += __builtin_amdgcn_logf(1.0f + y);
}

__device__ __forceinline__ float sigmoid_fast(float negz) {
  // 1/(1+e^{negz}) via the single-instruction v_rcp_f32.
  return __builtin_amdgcn_rcpf(1.0f + __expf(negz));
}

// 2-bit chunk XOR mask for the 64-B half-rows: rows sharing a bank base
// (r ≡ r' mod 4 within a 16-row group) get distinct chunks; interleaved
// lane groups are conflict-free by 16-dword row spacing.  Depends only on
// row bits 2-3, so fragment reads at row = base + mi*16 + fr share one
// per-lane mask.
__device__ __forceinline__ int kmask2(int r) { return (r >> 2) & 3; }

// Byte address of chunk c (0..7) of `row` inside one operand K-step image.
__device__ __forceinline__ int chunk_addr(int row, int c) {
  return (c >> 2) * HALF_BYTES + row * HROW + (((c & 3) ^ kmask2(row)) * 16);
}

// Register-staged fallback for edge blocks: same LDS image, zero-filled
// outside [rows, d).  Byte-based; k0/d in elements.
template <int EB>
__device__ __forceinline__ void stage_guarded(const char* __restrict__ gsrc,
                                              char* lds, int row0, int rows,
                                              int d, int k0) {
  const int t = threadIdx.x;
  const int row = t >> 1;          // 0..255
  const int ch0 = (t & 1) * 4;
  const int gr = row0 + row;
  const uint4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = ch0 + i;
    const int k = k0 + c * (16 / EB);        // element index of this chunk
    uint4 v = (gr < rows && k < d)
        ? *reinterpret_cast<const uint4*>(gsrc + (size_t)gr * d * EB + k * EB)
        : zero;
    *reinterpret_cast<uint4*>(lds + chunk_addr(row, c)) = v;
  }
}

// Optionally non-temporal store (flag bit 2): the g/gᵀ slabs are consumed
// later by the gradient GEMMs from L3/HBM, so nt stores skip the L2 and
// leave it to the operand panels.
template <bool NT, typename T>
__device__ __forceinline__ void st_g(T* p, T v) {
  if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

__device__ __forceinline__ i32x8 pack8(const uint4 lo, const uint4 hi) {
  return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
               (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// One bf16 K-half (32 elements): 32 MFMAs from the swizzled LDS image.
// SWAP exchanges the MFMA operands: the accumulators then hold the
// TRANSPOSED 16×16 fragments (row = lane&15 is the image row, the 4 regs are
// 4 consecutive text columns (lane>>4)*4+reg).  The k order inside each MFMA
// is unchanged, so every dot is the same sum in the same order.
template <bool SWAP>
__device__ __forceinline__ void mma_half_bf16(const char* smem, int aAddr,
                                              int bAddr,
                                              f32x4 (&acc)[FM][FN]) {
  bf16x8 afrag[FM], bfrag[FN];
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
    afrag[mi] = *reinterpret_cast<const bf16x8*>(
        smem + aAddr + mi * (16 * HROW));
#pragma unroll
  for (int ni = 0; ni < FN; ++ni)
    bfrag[ni] = *reinterpret_cast<const bf16x8*>(
        smem + bAddr + ni * (16 * HROW));
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
      acc[mi][ni] = SWAP
          ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                bfrag[ni], afrag[mi], acc[mi][ni], 0, 0, 0)
          : __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
}

// One fp8 K-step (128 elements): MX-scaled MFMA.  sA/sB are per-fragment
// scale dwords: unit (0x7f7f7f7f) for the per-tensor policy (scales folded
// into the temperature upstream), or per-ROW e8m0 bytes replicated across
// the dword for the row-wise policy (lane l of a fragment holds row
// lane&15, K-block lane>>4 — validated by tools/probe_mx_rowscale.hip) so
// the hardware emits the exact row-scaled dot.
__device__ __forceinline__ void mma_ktile_fp8(const char* smem,
                                              const int* aAddr,
                                              const int* bAddr,
                                              f32x4 (&acc)[FM][FN],
                                              const int* sA,
                                              const int* sB) {
  uint4 blo[FN], bhi[FN];
#pragma unroll
  for (int ni = 0; ni < FN; ++ni) {
    blo[ni] = *reinterpret_cast<const uint4*>(
        smem + bAddr[0] + ni * (16 * HROW));
    bhi[ni] = *reinterpret_cast<const uint4*>(
        smem + bAddr[1] + ni * (16 * HROW));
  }
#pragma unroll
  for (int mi = 0; mi < FM; ++mi) {
    const uint4 alo = *reinterpret_cast<const uint4*>(
        smem + aAddr[0] + mi * (16 * HROW));
    const uint4 ahi = *reinterpret_cast<const uint4*>(
        smem + aAddr[1] + mi * (16 * HROW));
    const i32x8 af = pack8(alo, ahi);
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
      acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          af, pack8(blo[ni], bhi[ni]), acc[mi][ni], 0, 0,
          0, sA[mi], 0, sB[ni]);
  }
}

// g-slab element bytes follow the compute dtype: bf16 kernels emit bf16 g,
// fp8 kernels emit e4m3 g (×448 fixed scale).
// SPLIT_POS (interior-only kernel): tiles that cannot hold a positive pair
// take an epilogue body compiled without the label predicate.
template <int MODE, bool INTERIOR, int EB, int EB_G = EB, bool NTG = false,
          bool GT_ALIGNED = false, bool RS = false, bool SPLIT_POS = false>
__device__ __forceinline__ void tile_body(
    const char* __restrict__ zimg, const char* __restrict__ ztxt,
    float t, float bias, float* __restrict__ out, __bf16* __restrict__ g_out,
    unsigned char* __restrict__ gt_out,
    const unsigned char* __restrict__ a_e8,
    const unsigned char* __restrict__ b_e8,
    const float* __restrict__ a_rat, const float* __restrict__ b_rat,
    int b, int n, int d, int ldg, int diag, int row_base, int col_base,
    char* smem) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wrow = (wave >> 2) * 128;   // wave sub-tile origin: 2×4 grid
  const int wcol = (wave & 3) * 64;
  // Where the bf16 LDS-staged g writeback is compiled in (g_lds16 below) the
  // MFMA operands are exchanged so a lane's 4 regs are 4 consecutive columns
  // of one g row: two packed converts + one ds_write_b64 per fragment.
  constexpr bool SWAP =
      (MODE != 0) && (EB == 2) && (EB_G == 2) && INTERIOR && GT_ALIGNED;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int KTE = 128 / EB;         // K elements per K-step
  const int ktiles = (d + KTE - 1) / KTE;
  const int fr = lane & 15;
  const int qbase = lane >> 4;          // chunk sub-index 0..3

  // Fragment read chunk pair: bf16 kk-half kk reads chunk kk*4+qbase; fp8
  // reads the two 16-B halves (chunks 2q, 2q+1) of its 32-element K-slice.
  int aAddr[2], bAddr[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int c = (EB == 2) ? (kk * 4 + qbase) : (qbase * 2 + kk);
    aAddr[kk] = chunk_addr(wrow + fr, c);
    bAddr[kk] = TILE_BYTES + chunk_addr(wcol + fr, c);
  }

  // fp8 MFMA scale dwords (per fragment, K-invariant: row-wise scales).
  int sA[FM], sB[FN];
  if (EB == 1) {
#pragma unroll
    for (int mi = 0; mi < FM; ++mi) {
      int e = 127;
      if (RS) {
        const int r = row_base + wrow + mi * 16 + (lane & 15);
        e = (INTERIOR || r < b) ? (int)a_e8[INTERIOR ? r : (r < b ? r : 0)]
                                : 127;
      }
      sA[mi] = 0x01010101 * e;
    }
#pragma unroll
    for (int ni = 0; ni < FN; ++ni) {
      int e = 127;
      if (RS) {
        const int c = col_base + wcol + ni * 16 + (lane & 15);
        e = (INTERIOR || c < n) ? (int)b_e8[INTERIOR ? c : (c < n ? c : 0)]
                                : 127;
      }
      sB[ni] = 0x01010101 * e;
    }
  }

  if (INTERIOR) {
    // DMA staging: one K-half of one operand = 16 KiB = 16 wave-instrs =
    // 2 per wave (16 rows each, 4 lanes per 64-B row).
    const int w = wave;
    const int rsub = lane >> 2;
    const int cch = lane & 3;
    int va[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rloc = (w * 2 + j) * 16 + rsub;
      va[j] = rloc * d * EB + ((cch ^ kmask2(rloc)) * 16);
    }
    const char* abase = zimg + (size_t)row_base * d * EB;
    const char* bbase = ztxt + (size_t)col_base * d * EB;

    // Stage K-half h of both operands into buffer buf (4 glds per wave).
    auto stage_half = [&](int buf, int h) {
      const int lb = __builtin_amdgcn_readfirstlane(w * 2048) +
          buf * (2 * TILE_BYTES) + h * HALF_BYTES;
      const int hoff = h * 64;          // K-half byte offset in the row
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        __builtin_amdgcn_global_load_lds(
            (gas_ptr)(abase + hoff + va[j]),
            (las_ptr)(smem + lb + j * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(
            (gas_ptr)(bbase + hoff + va[j]),
            (las_ptr)(smem + lb + TILE_BYTES + j * 1024), 16, 0, 0);
      }
    };
    auto advance = [&]() { abase += 128; bbase += 128; };

    stage_half(0, 0);
    stage_half(0, 1);
    advance();

    if (EB == 2) {
      // Half-granule schedule: the DMA of half h of tile k+1 is issued one
      // full iteration before its consumer, so each 16 KiB granule has a
      // whole iteration of wire time.  vmcnt counts per wave: 4 glds per
      // half; steady state keeps 2-3 halves in flight.
      for (int kt = 0; kt < ktiles; ++kt) {
        const bool more = kt + 1 < ktiles;
        if (more) {
          stage_half((kt + 1) & 1, 0);
          // outstanding: h1(kt) 4 + h0(kt+1) 4 → wait h0(kt)... h0(kt)
          // retired when ≤ 8 remain.
          asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        }
        __builtin_amdgcn_s_setprio(1);
        mma_half_bf16<SWAP>(smem, aAddr[0], bAddr[0], acc);
        __builtin_amdgcn_s_setprio(0);
        if (more) {
          stage_half((kt + 1) & 1, 1);
          advance();
          asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        }
        __builtin_amdgcn_s_setprio(1);
        mma_half_bf16<SWAP>(smem, aAddr[1], bAddr[1], acc);
        __builtin_amdgcn_s_setprio(0);
        aAddr[0] ^= 2 * TILE_BYTES; aAddr[1] ^= 2 * TILE_BYTES;
        bAddr[0] ^= 2 * TILE_BYTES; bAddr[1] ^= 2 * TILE_BYTES;
        // No end-of-iteration barrier: each half-region's write is already
        // fenced by the barrier in the OTHER half-phase — h0 of buf P is
        // last read before barrier B of the previous iteration and first
        // rewritten after it; h1 is last read before barrier A of this
        // iteration and rewritten after it.  (The ablation priced the
        // third barrier at ~7%.)
      }
    } else {
      // fp8: the single K=128 MFMA needs the whole K-step at once.
      for (int kt = 0; kt < ktiles; ++kt) {
        if (kt + 1 < ktiles) {
          stage_half((kt + 1) & 1, 0);
          stage_half((kt + 1) & 1, 1);
          advance();
          asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        }
        mma_ktile_fp8(smem, aAddr, bAddr, acc, sA, sB);
        aAddr[0] ^= 2 * TILE_BYTES; aAddr[1] ^= 2 * TILE_BYTES;
        bAddr[0] ^= 2 * TILE_BYTES; bAddr[1] ^= 2 * TILE_BYTES;
        asm volatile("s_barrier" ::: "memory");
      }
    }
  } else {
    stage_guarded<EB>(zimg, smem, row_base, b, d, 0);
    stage_guarded<EB>(ztxt, smem + TILE_BYTES, col_base, n, d, 0);
    __syncthreads();
    for (int kt = 0; kt < ktiles; ++kt) {
      if (kt + 1 < ktiles) {
        char* An = smem + ((kt + 1) & 1) * (2 * TILE_BYTES);
        stage_guarded<EB>(zimg, An, row_base, b, d, (kt + 1) * KTE);
        stage_guarded<EB>(ztxt, An + TILE_BYTES, col_base, n, d,
                          (kt + 1) * KTE);
      }
      if (EB == 2) {
        mma_half_bf16<SWAP>(smem, aAddr[0], bAddr[0], acc);
        mma_half_bf16<SWAP>(smem, aAddr[1], bAddr[1], acc);
      } else {
        mma_ktile_fp8(smem, aAddr, bAddr, acc, sA, sB);
      }
      aAddr[0] ^= 2 * TILE_BYTES; aAddr[1] ^= 2 * TILE_BYTES;
      bAddr[0] ^= 2 * TILE_BYTES; bAddr[1] ^= 2 * TILE_BYTES;
      __syncthreads();
    }
  }

  // Epilogue.  C/D layout (shape-determined, dtype-independent on gfx950):
  //   col = lane&15, row = (lane>>4)*4 + reg.
  // Per element: x = −l·z.  loss term = softplus(x); g = −l·σ(−l·z) =
  // ∓σ(x).  softplus and sigmoid share one exp: with y = e^{−|x|},
  // softplus(x) = max(x,0) + log(1+y) and σ(x) = (x≥0 ? 1 : y)/(1+y).
  // MODE 0 emits only the loss; MODE 1 only g + scalar partials; MODE 2
  // ("fwd+g") all three — the whole fwd+bwd recompute collapse costs one
  // extra log and the loss adds per lane.
  // With SWAP the fragment is transposed: row = lane&15, col = (lane>>4)*4
  // + reg.  lrow/lcol are the lane's coordinates of reg 0 in a fragment.
  //
  // Label predicate.  A tile can hold a positive only if the diagonal
  // segment [row_base + diag, row_base + diag + 255] meets its column range
  // (block-uniform; DIAG_NONE tested first, the sum is 64-bit).  At the
  // headline shape 16256 of 16384 tiles cannot: under SPLIT_POS they run a
  // body with no compare or select at all.  Otherwise the per-element test
  // gcol == grow + diag is one compare of the per-lane constant
  // dl = gcol0 − grow0 − diag with a compile-time fragment offset; dl =
  // INT_MIN (never matched, the offsets are within ±400) when the tile holds
  // no positive.
  const int lrow = SWAP ? (lane & 15) : (lane >> 4) * 4;
  const int lcol = SWAP ? (lane >> 4) * 4 : (lane & 15);
  const long long dlo = (long long)row_base + diag;
  const bool has_pos = (diag != DIAG_NONE) && (dlo + (BM - 1) >= col_base) &&
      (dlo <= (long long)col_base + (BN - 1));
  const int dl = has_pos
      ? (int)((long long)(col_base + wcol + lcol) -
              (long long)(row_base + wrow + lrow) - diag)
      : INT_MIN;
  float s_relu = 0.f, s_log2 = 0.f, s_gdot = 0.f, s_g = 0.f;
  if (MODE == 0) {
    auto body = [&](auto pc) __attribute__((always_inline)) {
      constexpr bool POS = decltype(pc)::value;
#pragma unroll
      for (int mi = 0; mi < FM; ++mi) {
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int grow = row_base + wrow + mi * 16 + lrow + reg;
            const int gcol = col_base + wcol + ni * 16 + lcol;
            if (INTERIOR || (grow < b && gcol < n)) {
              const float z = acc[mi][ni][reg] * t + bias;
              const bool pos = POS && (dl == mi * 16 + reg - ni * 16);
              const float x = pos ? -z : z;
              softplus_acc(x, __expf(-fabsf(x)), s_relu, s_log2);
            }
          }
        }
      }
    };
    if (SPLIT_POS && !has_pos) body(std::false_type{});
    else body(std::true_type{});
  } else {
    // One per-lane base offset + per-(mi,reg) scalar row offset keeps the
    // store addressing affine — per-element (size_t)grow*ldg math made the
    // allocator hoist 128 addresses and spill.  Caller guarantees
    // b*ldg*esz < 2^32 (ops/__init__.py column-chunks the slab).  ldg ≥ n
    // is the slab row stride — the ring strategy writes each received
    // chunk's g at its column offset inside one (b, W·b) slab.
    // bf16 path writes one bf16 slab; fp8 path writes e4m3 at a FIXED ×448
    // scale (|g| ≤ 1 by construction) AND a transposed (n, b) slab — both
    // consumed by torch._scaled_mm (mat1 must be row-major; a Python-side
    // 1-GB fp8 transpose measured ~5 ms, the fused stores are free).  The
    // 4 accumulator regs of a fragment are 4 consecutive gᵀ columns → one
    // packed 4-byte store.
    char* gb = reinterpret_cast<char*>(g_out) +
        ((size_t)row_base * ldg + col_base) * EB_G;
    const unsigned lane_off =
        (unsigned)(wrow + (lane >> 4) * 4) * (unsigned)ldg
        + (unsigned)(wcol + (lane & 15));
    unsigned char* gtb = gt_out +
        ((size_t)col_base * b + row_base);
    const unsigned lane_off_t =
        (unsigned)(wcol + (lane & 15)) * (unsigned)b
        + (unsigned)(wrow + (lane >> 4) * 4);
    // gᵀ staging (EB_G == 1, interior, b 16-aligned): the natural gᵀ store
    // is 4 B per lane at stride-b addresses — 16 different cache lines per
    // quarter-wave, measured as a ~0.6 ms store tail at B=32k.  Instead
    // stage the block's 256×256-byte gᵀ tile in LDS (the operand buffers
    // are dead once every wave reaches its epilogue) with a 2-bit row-seg
    // XOR swizzle, then write it back as coalesced dwordx4 columns.
    // GT_ALIGNED (b 16-aligned, checked by the caller) folds the choice at
    // compile time so the dead store path costs no registers — keeping both
    // paths live measured as an 80 B/lane spill.
    constexpr bool gt_lds = (EB_G == 1) && INTERIOR && GT_ALIGNED;
    unsigned* gt_img = reinterpret_cast<unsigned*>(smem);
    const int gsel = (wcol + (lane & 15)) & 3;
    const int gt_base0 = (wcol + (lane & 15)) * 64 + (lane >> 4);
    // The fp8 g slab gets the same treatment (1-B row-major scatter →
    // 64-KB LDS tile at smem+64K, byte writes merge per dword, dwordx4
    // row writeback); together with gt_img this uses the whole 128 KB.
    unsigned char* g_img = reinterpret_cast<unsigned char*>(smem) + 65536;
    const int g_base0 = (wrow + (lane >> 4) * 4) * 256 + wcol + (lane & 15);
    // bf16 g staging: the 256×256-element bf16 tile is exactly the whole
    // 128-KB smem (no gᵀ slab exists in bf16 mode).  The accumulators are
    // transposed here (SWAP), so a lane packs its 4 regs into ONE 8-B
    // ds_write_b64 at (row lane&15, 4 columns).  The 16-B chunk index is
    // XOR-ed with row&15: the 16 rows × 2 column quads of any half-wave
    // fill 256 contiguous-in-bank bytes, and the dwordx4 readback still
    // finds whole chunks.  The fragment column offset ni*32 B sits in
    // address bits 5-6, disjoint from the lane's own bits, so it folds
    // into the XOR as a compile-time constant.
    constexpr bool g_lds16 = SWAP;
    char* g_img16 = smem;
    const int g16_base0 = (wrow + (lane & 15)) * 512 +
        (((wcol + (lane >> 4) * 4) * 2) ^ ((lane & 15) << 4));
    if (gt_lds || g_lds16) __syncthreads();   // operand LDS reads complete
    // Row-wise policy: the saved slabs fold the OTHER side's scale ratio
    // (g slab ← text-row ratio for the dzimg GEMM, gᵀ slab ← image-row
    // ratio for the dztxt GEMM), each normalized by the tensor max scale
    // so |g·ratio| ≤ 1 keeps the fixed ×448 e4m3 packing exact; the
    // Python side multiplies the GEMM scale by s_ref/448.
    float rbv[FN];
#pragma unroll
    for (int ni = 0; ni < FN; ++ni) {
      rbv[ni] = 1.0f;
      if (RS && EB_G == 1) {
        const int c = col_base + wcol + ni * 16 + (lane & 15);
        rbv[ni] = (INTERIOR || c < n) ? b_rat[(INTERIOR || c < n) ? c : 0]
                                      : 0.0f;
      }
    }
    auto body = [&](auto pc) __attribute__((always_inline)) {
      constexpr bool POS = decltype(pc)::value;
#pragma unroll
      for (int mi = 0; mi < FM; ++mi) {
        float rav[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if (RS && EB_G == 1) {
          const int r0 = row_base + wrow + mi * 16 + (lane >> 4) * 4;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
            rav[rr] = (INTERIOR || r0 + rr < b)
                ? a_rat[(INTERIOR || r0 + rr < b) ? (r0 + rr) : 0] : 0.0f;
        }
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
          unsigned packed = 0;
          f32x4 gv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const int grow =
                row_base + wrow + mi * 16 + lrow + (SWAP ? 0 : reg);
            const int gcol =
                col_base + wcol + ni * 16 + lcol + (SWAP ? reg : 0);
            if (INTERIOR || (grow < b && gcol < n)) {
              const float dot = acc[mi][ni][reg];
              const float z = dot * t + bias;
              const bool pos = POS &&
                  (dl == mi * 16 - ni * 16 + (SWAP ? -reg : reg));
              const float x = pos ? -z : z;            // −l·z
              const float y = __expf(-fabsf(x));
              const float r = __builtin_amdgcn_rcpf(1.0f + y);
              if (MODE == 2) softplus_acc(x, y, s_relu, s_log2);
              const float sig = (x >= 0.0f) ? r : y * r;   // σ(x)
              const float g = pos ? -sig : sig;
              const unsigned row_off =
                  (unsigned)(mi * 16 + reg) * (unsigned)ldg;
              if (EB_G == 1) {
                const unsigned char q = __hip_fp8_e4m3(
                    (RS ? g * rbv[ni] : g) * 448.0f).__x;
                if (gt_lds)
                  g_img[g_base0 + (mi * 16 + reg) * 256 + ni * 16] = q;
                else
                  st_g<NTG>(reinterpret_cast<unsigned char*>(gb)
                                + lane_off + row_off + ni * 16, q);
                const unsigned char qt = RS
                    ? __hip_fp8_e4m3(g * rav[reg] * 448.0f).__x : q;
                packed |= (unsigned)qt << (8 * reg);
              } else if (g_lds16) {
                gv[reg] = g;
              } else {
                st_g<NTG>(reinterpret_cast<__bf16*>(gb)
                              + lane_off + row_off + ni * 16, (__bf16)g);
              }
              s_gdot += g * dot;
              s_g += g;
            }
          }
          if (g_lds16) {
            // 4 consecutive columns of row mi*16 + (lane&15): packed RNE
            // converts (same rounding as the scalar cast), one 8-B write.
            *reinterpret_cast<bf16x4*>(
                g_img16 + mi * (16 * 512) + (g16_base0 ^ (ni * 32))) =
                __builtin_convertvector(gv, bf16x4);
          }
          if (EB_G == 1) {
            const unsigned toff = lane_off_t
                + (unsigned)(ni * 16) * (unsigned)b + (unsigned)(mi * 16);
            if (gt_lds) {
              gt_img[gt_base0 + ni * 1024 +
                     ((((wrow >> 4) + mi) ^ gsel) << 2)] = packed;
            } else if (INTERIOR) {
              st_g<NTG>(reinterpret_cast<unsigned*>(gtb + toff), packed);
            } else {
              const int grow0 = row_base + wrow + mi * 16 + (lane >> 4) * 4;
              const int gcol = col_base + wcol + ni * 16 + (lane & 15);
              if (gcol < n)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                  if (grow0 + reg < b)
                    gtb[toff + reg] = (unsigned char)(packed >> (8 * reg));
            }
          }
        }
        // Cap epilogue register pressure.  The empty asm pins the running
        // sums here: without it the add chains were seen sunk past the
        // writeback in the general kernel (128 addends kept live, spilled).
        if (MODE == 2) asm volatile("" : "+v"(s_relu), "+v"(s_log2));
        asm volatile("" : "+v"(s_gdot), "+v"(s_g));
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (SPLIT_POS && !has_pos) body(std::false_type{});
    else body(std::true_type{});
    if (g_lds16) {
      // bf16 writeback: 8192 16-B chunks (8 elements of one row each),
      // nt dwordx4; the XOR swizzle is inverted per (row, chunk).
      __syncthreads();
#pragma unroll
      for (int sseg = 0; sseg < 16; ++sseg) {
        const int c = sseg * THREADS + threadIdx.x;
        const int row = c >> 5;
        const int cs = c & 31;
        const u32x4 v = *reinterpret_cast<const u32x4*>(
            g_img16 + row * 512 + ((cs ^ (row & 15)) * 16));
        st_g<true>(reinterpret_cast<u32x4*>(
                       gb + (size_t)row * (ldg * EB_G) + cs * 16), v);
      }
    }
    if (gt_lds) {
      // Coalesced writeback: 4096 16-B chunks per slab.  gᵀ: 16 rows of
      // one column each (swizzled); g: 16 columns of one row (row-major,
      // direct).  Consecutive threads cover consecutive chunks, dwordx4
      // global stores.
      __syncthreads();
#pragma unroll
      for (int sseg = 0; sseg < 8; ++sseg) {
        const int c = sseg * THREADS + threadIdx.x;
        const int col = c >> 4;
        const int rowseg = c & 15;
        const u32x4 v = *reinterpret_cast<const u32x4*>(
            gt_img + col * 64 + ((rowseg ^ (col & 3)) << 2));
        st_g<true>(reinterpret_cast<u32x4*>(
                       gtb + (size_t)col * b + rowseg * 16), v);
        const u32x4 w = *reinterpret_cast<const u32x4*>(
            g_img + col * 256 + rowseg * 16);
        st_g<true>(reinterpret_cast<u32x4*>(
                       gb + (size_t)col * ldg + rowseg * 16), w);
      }
    }
  }

  // Fold the tile's log2 sum into the loss partial: one multiply by ln 2.
  float s_loss = s_relu + LN2_F * s_log2;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    if (MODE != 1) s_loss += __shfl_down(s_loss, off);
    if (MODE != 0) {
      s_gdot += __shfl_down(s_gdot, off);
      s_g += __shfl_down(s_g, off);
    }
  }
  // Cross-wave reduction in LDS (the operand tiles are dead — every wave's
  // MFMA reads finished before its epilogue), then ONE atomic per scalar
  // per BLOCK into the block's XCD slot of the [8][32]-float output buffer.
  // Per-WAVE atomics to a single global line measured as a serialized
  // ~10 ns/op drain that dominated the fwd+g wall (3 × 131k ops ≈ +3 ms at
  // B=32k — all three fwd+g dtypes converged to the same ~5.7 ms floor);
  // per-block per-XCD 128-B slots cut the per-line rate ~384× and the
  // Python side sums the 256 floats once.
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
  if (lane == 0) {
    red[wave] = s_loss;
    red[8 + wave] = s_gdot;
    red[16 + wave] = s_g;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float r_loss = 0.f, r_gdot = 0.f, r_g = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      r_loss += red[w];
      r_gdot += red[8 + w];
      r_g += red[16 + w];
    }
    // Slot by the PRE-remap flat id: hardware dispatches block b to XCD
    // b % 8, so slots are XCD-local lines.
    const int slot =
        ((blockIdx.y * gridDim.x + blockIdx.x) & (NXCD - 1)) * OUT_STRIDE;
    // out layout per slot: [0] loss (MODE 0/2), [1] Σg·dot, [2] Σg
    // (MODE 1/2).
    if (MODE != 1) atomicAdd(&out[slot + 0], r_loss);
    if (MODE != 0) {
      atomicAdd(&out[slot + 1], r_gdot);
      atomicAdd(&out[slot + 2], r_g);
    }
  }
}

// Flat tile id (0 .. gx*gy-1) → tile coordinates under the remap flags.
__device__ __forceinline__ void remap_id(int flags, int id, int gx, int gy,
                                         int& bx, int& by) {
  if (flags & 1) {
    const int nwg = gx * gy;
    const int q = nwg / NXCD, r = nwg % NXCD;
    const int xcd = id % NXCD, idx = id / NXCD;
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  if (flags & 2) {
    // Group height selectable via flags bits 4-5 (00→8, 01→1, 10→4, 11→16)
    // for locality A/B experiments; 1 = band walk with the A panel
    // L2-resident for a whole XCD span.
    const int sel = (flags >> 4) & 3;
    const int gmh = sel == 0 ? GROUP_M : (sel == 1 ? 1 : (sel == 2 ? 4 : 16));
    const int group = id / (gmh * gy);
    const int within = id % (gmh * gy);
    const int gm = min(gmh, gx - group * gmh);
    bx = group * gmh + within % gm;
    by = within / gm;
  } else {
    bx = id % gx;
    by = id / gx;
  }
}

__device__ __forceinline__ void remap_block(int flags, int& bx, int& by) {
  remap_id(flags, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, gridDim.y,
           bx, by);
}

// Interior-only kernel: every tile full, d % K-step == 0, n%8==0 — checked
// by the host launcher.  Separate from the general kernel so the hot path's
// register allocation is not inflated by the guarded path.  Launched for
// the fp8 and e4m3-g instantiations; bf16 with bf16 g takes the persistent
// kernel below.
template <int MODE, int EB, int EB_G = EB, bool NTG = false, bool RS = false>
__launch_bounds__(THREADS) __global__ void siglip_tile_kernel_interior(
    const char* __restrict__ zimg, const char* __restrict__ ztxt,
    const float* __restrict__ t_prime, const float* __restrict__ bias_p,
    float* __restrict__ out, __bf16* __restrict__ g_out,
    unsigned char* __restrict__ gt_out,
    const unsigned char* __restrict__ a_e8,
    const unsigned char* __restrict__ b_e8,
    const float* __restrict__ a_rat, const float* __restrict__ b_rat,
    int b, int n, int d, int ldg, int diag, int flags) {
  __shared__ char smem[4 * TILE_BYTES];
  int bx, by;
  remap_block(flags, bx, by);
  const float t = __expf(*t_prime);
  const float bias = *bias_p;
  tile_body<MODE, true, EB, EB_G, NTG, true, RS, true>(
      zimg, ztxt, t, bias, out, g_out, gt_out, a_e8, b_e8, a_rat, b_rat,
      b, n, d, ldg, diag, bx * BM, by * BN, smem);
}

// General kernel: interior blocks take the DMA fast path, edge blocks the
// guarded register-staged path.  MODE 0: forward loss.  MODE 1: backward
// g-slab + scalar partials.
template <int MODE, int EB, int EB_G = EB, bool NTG = false, bool RS = false>
__launch_bounds__(THREADS) __global__ void siglip_tile_kernel(
    const char* __restrict__ zimg, const char* __restrict__ ztxt,
    const float* __restrict__ t_prime, const float* __restrict__ bias_p,
    float* __restrict__ out, __bf16* __restrict__ g_out,
    unsigned char* __restrict__ gt_out,
    const unsigned char* __restrict__ a_e8,
    const unsigned char* __restrict__ b_e8,
    const float* __restrict__ a_rat, const float* __restrict__ b_rat,
    int b, int n, int d, int ldg, int diag, int flags) {
  __shared__ char smem[4 * TILE_BYTES];
  int bx, by;
  remap_block(flags, bx, by);
  const int row_base = bx * BM;
  const int col_base = by * BN;

  const float t = __expf(*t_prime);
  const float bias = *bias_p;

  const bool interior = (row_base + BM <= b) && (col_base + BN <= n) &&
      (d % (128 / EB) == 0) && (n % 8 == 0);
  if (interior) {
    if ((EB_G == 1 && (b & 15) == 0 && (ldg & 15) == 0) ||
        (EB_G == 2 && MODE != 0 && (ldg & 7) == 0))
      tile_body<MODE, true, EB, EB_G, NTG, true, RS>(
          zimg, ztxt, t, bias, out, g_out, gt_out, a_e8, b_e8, a_rat, b_rat,
          b, n, d, ldg, diag, row_base, col_base, smem);
    else
      tile_body<MODE, true, EB, EB_G, NTG, false, RS>(
          zimg, ztxt, t, bias, out, g_out, gt_out, a_e8, b_e8, a_rat, b_rat,
          b, n, d, ldg, diag, row_base, col_base, smem);
  } else
    tile_body<MODE, false, EB, EB_G, NTG, false, RS>(
        zimg, ztxt, t, bias, out, g_out, gt_out, a_e8, b_e8, a_rat, b_rat,
        b, n, d, ldg, diag, row_base, col_base, smem);
}

// ---------------------------------------------------------------------------
// Persistent bf16 interior kernel (all three MODEs; bf16 g).  Same tile, same
// LDS operand image, same MFMA order and same per-element epilogue math as
// tile_body's interior bf16 path, but:
//   - workgroup w walks the flat tile ids w, w+G, w+2G, … (G = gridDim.x,
//     each id through remap_id).  With G % 8 == 0 a tile's id % 8 is still
//     the XCD it runs on, so the XCD-contiguous remap and the per-XCD scalar
//     slots keep their meaning.
//   - the K-loop is ONE stream across tiles: the last K-step of a tile
//     stages the first K-step of the next (new base pointers) where the
//     one-tile loop has "no more", so those granules are in flight before
//     the epilogue starts.  The buffer parity runs on through tile
//     boundaries (odd K-step counts flip it from tile to tile).
//   - the g writeback stages per WAVE in the 32 KiB above the operand
//     buffers (the kernel declares all 160 KiB): one 16-row × 128-B slice
//     per mi, two 2-KiB slots per wave so the writeback of slice mi overlaps
//     the math of mi+1.  A wave only reads what it wrote (LDS operations of
//     one wave execute in order), so the epilogue has no block-wide barrier
//     and never touches the operand buffers — which is what makes the early
//     prefetch legal.
//   - the scalar partials fold per tile into per-lane running sums; the wave
//     shuffle, the cross-wave LDS reduce and the three atomics run once per
//     WORKGROUP (adds in sequence: ≤128 per tile, ≤tiles-per-workgroup,
//     6 shuffle, 8 waves).
// Workgroups never wait on each other.
//
// vmcnt accounting.  The g stores count on the same vmcnt as the LDS-DMA
// loads.  The counted waits below are those of the one-tile loop, derived
// for loads alone: "at most k operations outstanding".  With stores in the
// count, at most k outstanding still implies at most k LOADS outstanding,
// and the loads complete in issue order among themselves (the one-tile loop
// relies on the same), so every wait still retires the granule it names:
// the stores can only make a wait stricter, never looser.  Nothing is
// assumed about the completion order of stores relative to loads.  The price
// is that the first two waits of a tile also wait for nearly all of the
// previous tile's g stores (the newly staged loads fill most of the k).
template <int MODE>
__launch_bounds__(THREADS) __global__ void siglip_tile_kernel_persistent(
    const char* __restrict__ zimg, const char* __restrict__ ztxt,
    const float* __restrict__ t_prime, const float* __restrict__ bias_p,
    float* __restrict__ out, __bf16* __restrict__ g_out,
    int d, int ldg, int diag, int flags, int gx, int gy) {
  __shared__ char smem[5 * TILE_BYTES];
  constexpr bool SWAP = MODE != 0;     // transposed fragments, see tile_body
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wrow = (wave >> 2) * 128;
  const int wcol = (wave & 3) * 64;
  const float t = __expf(*t_prime);
  const float bias = *bias_p;
  const int ktiles = d / 64;
  const int ntiles = gx * gy;
  const int G = gridDim.x;

  const int fr = lane & 15;
  const int qbase = lane >> 4;
  int aAddr[2], bAddr[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    aAddr[kk] = chunk_addr(wrow + fr, kk * 4 + qbase);
    bAddr[kk] = TILE_BYTES + chunk_addr(wcol + fr, kk * 4 + qbase);
  }

  // DMA staging, as in tile_body.
  const int rsub = lane >> 2;
  const int cch = lane & 3;
  int va[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int rloc = (wave * 2 + j) * 16 + rsub;
    va[j] = rloc * d * 2 + ((cch ^ kmask2(rloc)) * 16);
  }
  const char* abase;
  const char* bbase;
  auto stage_half = [&](int buf, int h) {
    const int lb = __builtin_amdgcn_readfirstlane(wave * 2048) +
        buf * (2 * TILE_BYTES) + h * HALF_BYTES;
    const int hoff = h * 64;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      __builtin_amdgcn_global_load_lds(
          (gas_ptr)(abase + hoff + va[j]),
          (las_ptr)(smem + lb + j * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(
          (gas_ptr)(bbase + hoff + va[j]),
          (las_ptr)(smem + lb + TILE_BYTES + j * 1024), 16, 0, 0);
    }
  };

  // Per-wave g staging: slot s of this wave at stg + s*2048, row r at
  // r*128, 16-B chunk c at (c ^ ((r>>1)&7))*16 — rows r, r+1 (r even) share
  // a mask and fill one 256-B bank row, so the 16 rows × 2 column quads of a
  // half-wave's 8-B writes and the 2 rows × 8 chunks of a quarter-wave's
  // 16-B reads are conflict-free.  Write: lane holds row lane&15, columns
  // ni*16 + (lane>>4)*4 .. +3 → chunk ni*2 + (lane>>5), half (lane>>4)&1;
  // ni sits in chunk bits 1-2 and folds into the XOR as a constant.  Read /
  // store: 16-B unit u = j*64 + lane → row u>>3, chunk u&7.
  char* stg = smem + 4 * TILE_BYTES + wave * 4096;
  const int wr0 = fr * 128 + (((lane >> 5) ^ ((fr >> 1) & 7)) << 4) +
      ((lane >> 4) & 1) * 8;
  int rd[2];
  unsigned goff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int u = j * 64 + lane;
    const int r = u >> 3, c = u & 7;
    rd[j] = r * 128 + ((c ^ ((r >> 1) & 7)) << 4);
    goff[j] = ((unsigned)(wrow + r) * (unsigned)ldg + (unsigned)wcol) * 2u +
        (unsigned)c * 16u;
  }

  const int lrow = SWAP ? fr : qbase * 4;
  const int lcol = SWAP ? qbase * 4 : fr;

  int tile = blockIdx.x;
  int bx, by;
  remap_id(flags, tile, gx, gy, bx, by);
  int row_base = bx * BM, col_base = by * BN;
  abase = zimg + (size_t)row_base * d * 2;
  bbase = ztxt + (size_t)col_base * d * 2;
  stage_half(0, 0);
  stage_half(0, 1);
  abase += 128; bbase += 128;
  int nbuf = 1;                       // buffer the next K-step is staged to

  float w_loss = 0.f, w_gdot = 0.f, w_g = 0.f;   // per-workgroup running sums
  for (;;) {
    const int next = tile + G;
    const bool has_next = next < ntiles;
    int nrow = 0, ncol = 0;
    if (has_next) {
      remap_id(flags, next, gx, gy, bx, by);
      nrow = bx * BM; ncol = by * BN;
    }

    f32x4 acc[FM][FN];
#pragma unroll
    for (int mi = 0; mi < FM; ++mi)
#pragma unroll
      for (int ni = 0; ni < FN; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < ktiles; ++kt) {
      const bool last = kt + 1 == ktiles;
      const bool more = !last || has_next;
      if (last && has_next) {          // next K-step = first of the next tile
        abase = zimg + (size_t)nrow * d * 2;
        bbase = ztxt + (size_t)ncol * d * 2;
      }
      if (more) {
        stage_half(nbuf, 0);
        // loads outstanding: h0(kt) h1(kt) h0(kt+1) = 12; ≤ 8 outstanding
        // in all ⇒ ≤ 8 loads ⇒ h0(kt) retired (stores only tighten this).
        asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
      } else {
        // h0(kt) h1(kt) = 8 loads; ≤ 4 outstanding ⇒ h0(kt) retired.
        asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
      }
      __builtin_amdgcn_s_setprio(1);
      mma_half_bf16<SWAP>(smem, aAddr[0], bAddr[0], acc);
      __builtin_amdgcn_s_setprio(0);
      if (more) {
        stage_half(nbuf, 1);
        abase += 128; bbase += 128;
        // loads outstanding: h1(kt) h0(kt+1) h1(kt+1) = 12; ≤ 8 ⇒ h1(kt)
        // retired.
        asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      }
      __builtin_amdgcn_s_setprio(1);
      mma_half_bf16<SWAP>(smem, aAddr[1], bAddr[1], acc);
      __builtin_amdgcn_s_setprio(0);
      aAddr[0] ^= 2 * TILE_BYTES; aAddr[1] ^= 2 * TILE_BYTES;
      bAddr[0] ^= 2 * TILE_BYTES; bAddr[1] ^= 2 * TILE_BYTES;
      nbuf ^= 1;
      // Buffer reuse is fenced exactly as in the one-tile loop: the
      // epilogue adds no barrier and touches no operand buffer.
    }

    // Epilogue (see tile_body for the math and the label predicate).
    const long long dlo = (long long)row_base + diag;
    const bool has_pos = (diag != DIAG_NONE) &&
        (dlo + (BM - 1) >= col_base) &&
        (dlo <= (long long)col_base + (BN - 1));
    const int dl = has_pos
        ? (int)((long long)(col_base + wcol + lcol) -
                (long long)(row_base + wrow + lrow) - diag)
        : INT_MIN;
    float s_relu = 0.f, s_log2 = 0.f, s_gdot = 0.f, s_g = 0.f;
    char* gb = reinterpret_cast<char*>(g_out) +
        ((size_t)row_base * ldg + col_base) * 2;
    auto body = [&](auto pc) __attribute__((always_inline)) {
      constexpr bool POS = decltype(pc)::value;
      u32x4 pend[2];
      auto store_slice = [&](int m) __attribute__((always_inline)) {
        char* gbm = gb + (size_t)(m * 16) * ((size_t)ldg * 2);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          st_g<true>(reinterpret_cast<u32x4*>(gbm + goff[j]), pend[j]);
      };
#pragma unroll
      for (int mi = 0; mi < FM; ++mi) {
        char* slot = stg + (mi & 1) * 2048;
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
          f32x4 gv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            const float dot = acc[mi][ni][reg];
            const float z = dot * t + bias;
            const bool pos = POS &&
                (dl == mi * 16 - ni * 16 + (SWAP ? -reg : reg));
            const float x = pos ? -z : z;            // −l·z
            const float y = __expf(-fabsf(x));
            if (MODE != 1) softplus_acc(x, y, s_relu, s_log2);
            if (MODE != 0) {
              const float r = __builtin_amdgcn_rcpf(1.0f + y);
              const float sig = (x >= 0.0f) ? r : y * r;   // σ(x)
              const float g = pos ? -sig : sig;
              gv[reg] = g;
              s_gdot += g * dot;
              s_g += g;
            }
          }
          if (MODE != 0)
            *reinterpret_cast<bf16x4*>(slot + (wr0 ^ (ni * 32))) =
                __builtin_convertvector(gv, bf16x4);
        }
        if (MODE != 0) {
          // Store slice mi-1 (read back one iteration ago, so its LDS
          // latency hid under this slice's math), then read this slice
          // back as whole 128-B rows: the wave reads only what it wrote.
          if (mi > 0) store_slice(mi - 1);
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int j = 0; j < 2; ++j)
            pend[j] = *reinterpret_cast<const u32x4*>(slot + rd[j]);
          if (mi == FM - 1) store_slice(mi);
          asm volatile("" : "+v"(s_gdot), "+v"(s_g));
        }
        if (MODE != 1) asm volatile("" : "+v"(s_relu), "+v"(s_log2));
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    if (!has_pos) body(std::false_type{});
    else body(std::true_type{});
    w_loss += s_relu + LN2_F * s_log2;
    w_gdot += s_gdot;
    w_g += s_g;

    if (!has_next) break;
    tile = next; row_base = nrow; col_base = ncol;
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    if (MODE != 1) w_loss += __shfl_down(w_loss, off);
    if (MODE != 0) {
      w_gdot += __shfl_down(w_gdot, off);
      w_g += __shfl_down(w_g, off);
    }
  }
  // Once per workgroup: cross-wave reduce in the staging region (no DMA is
  // in flight after the last tile's vmcnt(0)), one atomic per scalar into
  // the workgroup's XCD slot.
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem + 4 * TILE_BYTES);
  if (lane == 0) {
    red[wave] = w_loss;
    red[8 + wave] = w_gdot;
    red[16 + wave] = w_g;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float r_loss = 0.f, r_gdot = 0.f, r_g = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      r_loss += red[w];
      r_gdot += red[8 + w];
      r_g += red[16 + w];
    }
    const int slot = (blockIdx.x & (NXCD - 1)) * OUT_STRIDE;
    if (MODE != 1) atomicAdd(&out[slot + 0], r_loss);
    if (MODE != 0) {
      atomicAdd(&out[slot + 1], r_gdot);
      atomicAdd(&out[slot + 2], r_g);
    }
  }
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------
// Fused row-wise L2 normalize (bf16 in/out, fp32 math) — replaces the
// F.normalize autograd chain in the towers (measured 0.29 ms fwd+bwd per
// tower at (32768, 768) as ~10 stock elementwise/reduce kernels; these two
// single-pass kernels do the same work at memory speed).
//   fwd: y = x / max(‖x‖₂, eps)  (torch F.normalize semantics), saves
//        rn = 1/max(‖x‖₂, eps)
//   bwd: dx = rn · (dy − y · ⟨y, dy⟩)   per row
// One wave per row, 8 rows per 512-thread block, bf16-pair loads.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

__launch_bounds__(512) __global__ void l2norm_fwd_kernel(
    const __bf16* __restrict__ x, __bf16* __restrict__ y,
    float* __restrict__ rn, int b, int d, float eps) {
  const int row = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (row >= b) return;
  const int lane = threadIdx.x & 63;
  const bf16x2* xr = reinterpret_cast<const bf16x2*>(x + (size_t)row * d);
  const int dp = d >> 1;
  float s = 0.f;
  for (int k = lane; k < dp; k += 64) {
    const bf16x2 v = xr[k];
    const float a0 = (float)v.x, a1 = (float)v.y;
    s += a0 * a0 + a1 * a1;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) s += __shfl_down(s, off);
  const float r = 1.0f / fmaxf(sqrtf(__shfl(s, 0)), eps);
  bf16x2* yr = reinterpret_cast<bf16x2*>(y + (size_t)row * d);
  for (int k = lane; k < dp; k += 64) {
    const bf16x2 v = xr[k];
    bf16x2 o;
    o.x = (__bf16)((float)v.x * r);
    o.y = (__bf16)((float)v.y * r);
    yr[k] = o;
  }
  if (lane == 0) rn[row] = r;
}

__launch_bounds__(512) __global__ void l2norm_bwd_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ y,
    const float* __restrict__ rn, __bf16* __restrict__ dx, int b, int d) {
  const int row = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (row >= b) return;
  const int lane = threadIdx.x & 63;
  const bf16x2* dyr = reinterpret_cast<const bf16x2*>(dy + (size_t)row * d);
  const bf16x2* yr = reinterpret_cast<const bf16x2*>(y + (size_t)row * d);
  const int dp = d >> 1;
  float dot = 0.f;
  for (int k = lane; k < dp; k += 64) {
    const bf16x2 a = dyr[k], c = yr[k];
    dot += (float)a.x * (float)c.x + (float)a.y * (float)c.y;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) dot += __shfl_down(dot, off);
  dot = __shfl(dot, 0);
  const float r = rn[row];
  bf16x2* dxr = reinterpret_cast<bf16x2*>(dx + (size_t)row * d);
  for (int k = lane; k < dp; k += 64) {
    const bf16x2 a = dyr[k], c = yr[k];
    bf16x2 o;
    o.x = (__bf16)(r * ((float)a.x - (float)c.x * dot));
    o.y = (__bf16)(r * ((float)a.y - (float)c.y * dot));
    dxr[k] = o;
  }
}

template <int MODE, int EB, int EB_G = EB, bool NTG = false, bool RS = false>
int launch_nt(uintptr_t stream, const void* zimg, const void* ztxt,
              const void* t_prime, const void* bias, void* out, void* g_out,
              void* gt_out, const void* a_e8, const void* b_e8,
              const void* a_rat, const void* b_rat, int b, int n, int d,
              int ldg, int diag, int flags) {
  dim3 grid(ceil_div(b, BM), ceil_div(n, BN));
  // The interior-only kernel folds the LDS-staged g/gᵀ writeback at compile
  // time (GT_ALIGNED), which needs 16-aligned slab strides for its dwordx4
  // stores — odd ldg shapes take the general kernel's guarded dispatch.
  const bool interior = (b % BM == 0) && (n % BN == 0) &&
      (d % (128 / EB) == 0) &&
      (EB_G == 1 ? (ldg & 15) == 0 : (MODE == 0 || (ldg & 7) == 0));
  if constexpr (EB == 2 && EB_G == 2) {
    if (interior) {
      // Persistent grid: min(tiles, CUs) workgroups (one fits per CU: 160 KiB
      // LDS), rounded down to a multiple of 8 above 8 so that tile id % 8
      // stays the XCD.  flags bits 8-23: workgroup cap (0 = automatic, for
      // tests and sweeps); bit 24: one tile per workgroup, same kernel (A/B).
      static int n_cu = 0;
      if (n_cu == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount,
                                  dev) != hipSuccess || n_cu <= 0)
          return (int)hipErrorInvalidDevice;
      }
      const int tiles = (int)(grid.x * grid.y);
      const int cap = (flags >> 8) & 0xffff;
      int wgs = tiles;
      if (!(flags & (1 << 24))) {
        wgs = cap ? cap : n_cu;
        if (wgs > tiles) wgs = tiles;
        if (wgs > 8) wgs -= wgs % 8;
      }
      hipLaunchKernelGGL(
          (siglip_tile_kernel_persistent<MODE>), dim3(wgs), dim3(THREADS), 0,
          (hipStream_t)stream, (const char*)zimg, (const char*)ztxt,
          (const float*)t_prime, (const float*)bias, (float*)out,
          (__bf16*)g_out, d, ldg, diag, flags, (int)grid.x, (int)grid.y);
      return (int)hipGetLastError();
    }
  } else if (interior) {
    hipLaunchKernelGGL(
        (siglip_tile_kernel_interior<MODE, EB, EB_G, NTG, RS>),
        grid, dim3(THREADS), 0, (hipStream_t)stream,
        (const char*)zimg, (const char*)ztxt,
        (const float*)t_prime, (const float*)bias,
        (float*)out, (__bf16*)g_out, (unsigned char*)gt_out,
        (const unsigned char*)a_e8, (const unsigned char*)b_e8,
        (const float*)a_rat, (const float*)b_rat,
        b, n, d, ldg, diag, flags);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(
      (siglip_tile_kernel<MODE, EB, EB_G, NTG, RS>), grid, dim3(THREADS),
      0, (hipStream_t)stream,
      (const char*)zimg, (const char*)ztxt,
      (const float*)t_prime, (const float*)bias,
      (float*)out, (__bf16*)g_out, (unsigned char*)gt_out,
      (const unsigned char*)a_e8, (const unsigned char*)b_e8,
      (const float*)a_rat, (const float*)b_rat,
      b, n, d, ldg, diag, flags);
  return (int)hipGetLastError();
}

template <int MODE, int EB, int EB_G = EB>
int launch(uintptr_t stream, const void* zimg, const void* ztxt,
           const void* t_prime, const void* bias, void* out, void* g_out,
           void* gt_out, int b, int n, int d, int ldg, int diag, int flags,
           const void* a_e8 = nullptr, const void* b_e8 = nullptr,
           const void* a_rat = nullptr, const void* b_rat = nullptr) {
  if (b <= 0 || n <= 0) return (int)hipSuccess;
  if (d % (16 / EB) != 0 || ldg < n) return (int)hipErrorInvalidValue;
  const bool rs = (EB == 1) && a_e8 != nullptr;
  if (rs && MODE != 0 && (a_rat == nullptr || b_rat == nullptr))
    return (int)hipErrorInvalidValue;
  if (rs)
    return launch_nt<MODE, EB, EB_G, false, true>(
        stream, zimg, ztxt, t_prime, bias, out, g_out, gt_out, a_e8, b_e8,
        a_rat, b_rat, b, n, d, ldg, diag, flags);
  if (MODE != 0 && (flags & 4))
    return launch_nt<MODE, EB, EB_G, true>(
        stream, zimg, ztxt, t_prime, bias, out, g_out, gt_out, a_e8, b_e8,
        a_rat, b_rat, b, n, d, ldg, diag, flags);
  return launch_nt<MODE, EB, EB_G, false>(
      stream, zimg, ztxt, t_prime, bias, out, g_out, gt_out, a_e8, b_e8,
      a_rat, b_rat, b, n, d, ldg, diag, flags);
}

}  // namespace

extern "C" {

int siglip_ext_abi(void) { return 13; }

// Fused per-tensor fp8-e4m3 quantization: one amax pass (block reduce +
// one atomicMax of the float bits per block — positive floats order as
// uints) and one cast pass reading the amax from device memory (no host
// sync).  Replaces ~5 stock kernels / ~0.25 ms per quantize-pair at B=32k.

__launch_bounds__(256) __global__ void amax_abs_bf16_kernel(
    const __bf16* __restrict__ x, unsigned* __restrict__ amax_bits,
    long long n) {
  float m = 0.f;
  const long long stride = (long long)gridDim.x * 256 * 8;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
       i < n; i += stride) {
    if (i + 8 <= n) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i);
#pragma unroll
      for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf((float)v[k]));
    } else {
      for (long long j = i; j < n; ++j) m = fmaxf(m, fabsf((float)x[j]));
    }
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_down(m, off));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(amax_bits, __float_as_uint(m));
  }
}

__launch_bounds__(256) __global__ void quant_fp8_bf16_kernel(
    const __bf16* __restrict__ x, unsigned char* __restrict__ q,
    float* __restrict__ scale_out, const unsigned* __restrict__ amax_bits,
    long long n) {
  const float amax = fmaxf(__uint_as_float(*amax_bits), 9.5367431640625e-7f);
  const float r = 448.0f / amax;
  if (blockIdx.x == 0 && threadIdx.x == 0) *scale_out = amax / 448.0f;
  const long long stride = (long long)gridDim.x * 256 * 8;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
       i < n; i += stride) {
    if (i + 8 <= n) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(x + i);
      unsigned lo = 0, hi = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        lo |= (unsigned)__hip_fp8_e4m3((float)v[k] * r).__x << (8 * k);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        hi |= (unsigned)__hip_fp8_e4m3((float)v[4 + k] * r).__x << (8 * k);
      *reinterpret_cast<uint2*>(q + i) = {lo, hi};
    } else {
      for (long long j = i; j < n; ++j)
        q[j] = __hip_fp8_e4m3((float)x[j] * r).__x;
    }
  }
}

// Row-wise pow2 (e8m0) quantization for the hardware-scaled MX path:
// per row, k = ceil(log2(amax/448)), e8m0 byte = 127+k, q = x·2^-k (so
// |q| ≤ 448 uses the full e4m3 range and the MFMA's 2^(e-127) dequant is
// exact).  Also maintains the tensor-max exponent (atomicMax) for the
// backward-fold normalization.  One wave per row.
__launch_bounds__(512) __global__ void quant_fp8_rowwise_kernel(
    const __bf16* __restrict__ x, unsigned char* __restrict__ q,
    unsigned char* __restrict__ e8, int* __restrict__ emax,
    int b, int d) {
  // Grid-strided rows: one row per wave per iteration; a bounded grid
  // keeps each wave looping (amortizes launch/drain and pipelines the
  // per-row dependent load→reduce→convert chain across iterations).
  const int lane = threadIdx.x & 63;
  const int rstep = gridDim.x * 8;
  int emax_loc = 0;
  for (int row = blockIdx.x * 8 + (threadIdx.x >> 6); row < b;
       row += rstep) {
  const __bf16* xr = x + (size_t)row * d;
  const bf16x8* xr8 = reinterpret_cast<const bf16x8*>(xr);
  // vector path needs 16-B row alignment: d % 8 (rows then stay aligned)
  const int d8 = ((d & 7) == 0) ? (d >> 3) : 0;
  float m = 0.f;
  for (int k = lane; k < d8; k += 64) {
    const bf16x8 v = xr8[k];
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)v[e]));
  }
  for (int k = (d8 << 3) + lane; k < d; k += 64)
    m = fmaxf(m, fabsf((float)xr[k]));
#pragma unroll
  for (int off = 32; off; off >>= 1) m = fmaxf(m, __shfl_down(m, off));
  m = __shfl(m, 0);
  const float t = fmaxf(m, 1e-30f) / 448.0f;
  const unsigned bits = __float_as_uint(t);
  int k2 = (int)((bits >> 23) & 0xff) - 127 + ((bits & 0x7fffffu) ? 1 : 0);
  if (k2 < -126) k2 = -126;
  if (k2 > 127) k2 = 127;
  const float r = __uint_as_float((unsigned)(127 - k2) << 23);   // 2^-k
  unsigned char* qr = q + (size_t)row * d;
  for (int k = lane; k < d8; k += 64) {
    const bf16x8 v = xr8[k];
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      lo |= (unsigned)__hip_fp8_e4m3((float)v[e] * r).__x << (8 * e);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      hi |= (unsigned)__hip_fp8_e4m3((float)v[4 + e] * r).__x << (8 * e);
    reinterpret_cast<uint2*>(qr)[k] = {lo, hi};
  }
  for (int k = (d8 << 3) + lane; k < d; k += 64)
    qr[k] = __hip_fp8_e4m3((float)xr[k] * r).__x;
  if (lane == 0) {
    e8[row] = (unsigned char)(127 + k2);
    if (127 + k2 > emax_loc) emax_loc = 127 + k2;
  }
  }
  if (lane == 0 && emax_loc > 0) atomicMax(emax, emax_loc);
}

int quant_fp8_rowwise_bf16(uintptr_t stream, const void* x, void* q,
                           void* e8, void* emax, int b, int d) {
  if (b <= 0 || d <= 0) return (int)hipErrorInvalidValue;
  const int blocks = ceil_div(b, 8) < 1024 ? ceil_div(b, 8) : 1024;
  hipLaunchKernelGGL(quant_fp8_rowwise_kernel, dim3(blocks),
                     dim3(512), 0, (hipStream_t)stream, (const __bf16*)x,
                     (unsigned char*)q, (unsigned char*)e8, (int*)emax,
                     b, d);
  return (int)hipGetLastError();
}

int l2norm_fwd_bf16(uintptr_t stream, const void* x, void* y, void* rn,
                    int b, int d, float eps) {
  if (b <= 0) return (int)hipSuccess;
  if (d <= 0 || (d & 1)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(l2norm_fwd_kernel, dim3(ceil_div(b, 8)), dim3(512), 0,
                     (hipStream_t)stream, (const __bf16*)x, (__bf16*)y,
                     (float*)rn, b, d, eps);
  return (int)hipGetLastError();
}

int l2norm_bwd_bf16(uintptr_t stream, const void* dy, const void* y,
                    const void* rn, void* dx, int b, int d) {
  if (b <= 0) return (int)hipSuccess;
  if (d <= 0 || (d & 1)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(ceil_div(b, 8)), dim3(512), 0,
                     (hipStream_t)stream, (const __bf16*)dy,
                     (const __bf16*)y, (const float*)rn, (__bf16*)dx, b, d);
  return (int)hipGetLastError();
}

// Per-tensor e4m3 quantization.  amax_bits must be a zeroed 4-B buffer;
// q gets n e4m3 bytes, scale_out the fp32 scale (x ≈ q · scale).
// n must be a multiple of 8 for the vectorized path to cover all of it
// exactly when (x, q) are 16-B aligned; any n works (tail loop).
int quant_fp8_bf16(uintptr_t stream, const void* x, void* q,
                   void* scale_out, void* amax_bits, long long n) {
  if (n <= 0) return (int)hipSuccess;
  const int blocks = 2048;
  hipLaunchKernelGGL(amax_abs_bf16_kernel, dim3(blocks), dim3(256), 0,
                     (hipStream_t)stream, (const __bf16*)x,
                     (unsigned*)amax_bits, n);
  hipLaunchKernelGGL(quant_fp8_bf16_kernel, dim3(blocks), dim3(256), 0,
                     (hipStream_t)stream, (const __bf16*)x,
                     (unsigned char*)q, (float*)scale_out,
                     (const unsigned*)amax_bits, n);
  return (int)hipGetLastError();
}

// The single tile-kernel entry point.  (mode, eb, eb_g) selects one of the
// eight instantiated combinations of tile_body's template parameters:
//   mode  0 = fwd (loss only), 1 = bwd-g (recompute: g slab + scalar
//         partials), 2 = fwd+g ("saved-g": loss, g slab and both partials in
//         one pass, so backward is pure GEMMs);
//   eb    logit operand bytes: 2 = bf16, 1 = e4m3;
//   eb_g  g-slab element bytes: 2 = bf16 g only, 1 = e4m3 x448 g AND its
//         transpose gt (n, b) for the fp8 gradient GEMMs.
//         (eb, eb_g) = (2, 1) is the "mixed" policy.
// `out` is a zeroed float[8][32] per-XCD-slot buffer, slot layout
// {loss, sum g*dot, sum g}; the caller sums slots.  `ldg` is the g-slab row
// stride in elements (>= n), so the ring strategy can write each chunk at
// its column offset inside one (b, W*b) slab.  The four row-scale pointers
// select the fp8 policy: null = per-tensor (scales folded into the
// temperature upstream); non-null = row-wise e8m0 hardware dequant
// (a_e8/b_e8: per-row exponent bytes; a_rat/b_rat: fp32 per-row scale /
// tensor-max scale, consumed by the slab folds in modes 1/2).
int siglip_tile(uintptr_t stream, int mode, int eb, int eb_g,
                const void* zimg, const void* ztxt, const void* t_prime,
                const void* bias, void* out, void* g_out, void* gt_out,
                const void* a_e8, const void* b_e8, const void* a_rat,
                const void* b_rat, int b, int n, int d, int ldg, int diag,
                int flags) {
  // Argument checks, before any HIP call.  The g-emitting modes need their
  // slabs; the e4m3 slab pair additionally needs b % 4 (packed 4-B gt
  // stores).  Mode 0 writes no slab, so (0, 1, 1) takes any b.
  if (mode != 0 && g_out == nullptr) return (int)hipErrorInvalidValue;
  if (mode != 0 && eb_g == 1 && (gt_out == nullptr || b % 4 != 0))
    return (int)hipErrorInvalidValue;
#define SIGLIP_TILE_CASE(M, EB, EB_G)                                       \
  if (mode == M && eb == EB && eb_g == EB_G)                                \
    return launch<M, EB, EB_G>(stream, zimg, ztxt, t_prime, bias, out,      \
                               g_out, gt_out, b, n, d, ldg, diag, flags,    \
                               a_e8, b_e8, a_rat, b_rat)
  SIGLIP_TILE_CASE(0, 2, 2);
  SIGLIP_TILE_CASE(1, 2, 2);
  SIGLIP_TILE_CASE(0, 1, 1);
  SIGLIP_TILE_CASE(1, 2, 1);
  SIGLIP_TILE_CASE(1, 1, 1);
  SIGLIP_TILE_CASE(2, 2, 2);
  SIGLIP_TILE_CASE(2, 2, 1);
  SIGLIP_TILE_CASE(2, 1, 1);
#undef SIGLIP_TILE_CASE
  return (int)hipErrorInvalidValue;
}

}  // extern "C"
