// Training path, the weight-gradient stage: the parameter part of loss.backward() (src/train.py:90):
// dW[n][k] = sum_m dpre[m][n] x[m][k] (+ the bias column) over the batch, chunked over samples, each
// chunk's partial reduced in a fixed order (deterministic).  Chunk policy, workspace sizers and
// the route of a launch: wgrad_plan.h; the job descriptor and the launchers' prototypes:
// train_internal.h; who launches what per parameter: train_api.hip (param_grads).
//
//   wgrad_kernel, wgrad_lds_kernel      fp32 MFMA (nerf_arith F32): unaligned fallback, LDS-staged
//   wgrad_bf_kernel, wgrad_bf_k64_kernel  bf16x6, the split arithmetic's GEMMs outside the whole tile
//                                       (generic tiles / 256 x (K <= 64))
//   wgrad_h16w_kernel, wgrad_h16h_kernel  split f16, the 256 x 256 whole tile: one workgroup per
//                                       chunk / two half-tile workgroups per CU on tile-major rows
//   wgrad_pair16_kernel                 layer 0 + the skip layer's PE columns, split f16
//   wgrad_head3_kernel                  the rgb head's 3 rows, streaming (+ the fused per-ray sums)
//   wgrad_reduce_kernel                 the chunk partials, in double, rounded once
//   app_grad_kernel, ray_sums_kernel    appearance-embedding gradient, per-ray gradient sums
#include "train_internal.h"
#include "stream16.h"

namespace nerf {

// ---------------------------------------------------------------------------------- wgrad
// partial[c][n*KP + k'] = sum over samples m of chunk c of a[m][n] * x'[m][k'], k' < KP = K + 1,
// where x'[m][k] = x[xrow(m)][k] for k < K and x'[m][K] = 1 (the bias column).  xrow(m) = m / x_div
// (x_div = 1: a per-sample input; = N: a per-ray input; 0: one broadcast row).  Each chunk's
// partial occupies wgrad_stride(N, K) floats (N*KP rounded up to 4, for 16-byte reduce loads, + 4).
// A chunk is kWChunk samples or the policy's wgrad_chunk_len (wgrad_plan.h).

// Row of a 32 x 32 MFMA accumulator tile that register g holds in lane half h (layout.h).
__device__ __forceinline__ int acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

// Fallback (unaligned operands): one wave per 32 (n) x 64 (k') tile of one chunk, operands
// loaded straight from global memory (A = a^T fragment: n = l&31, sample = l>>5; B = x'
// fragment: sample = l>>5, k = l&31).
__global__ void __launch_bounds__(256)
wgrad_kernel(const float* __restrict__ a, int64_t lda, int N, const float* __restrict__ x, int64_t ldx, int K,
             int64_t x_div, int64_t M, float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int KP = K + 1;
  const int ntn = (N + 31) / 32, ntk = (KP + 63) / 64;
  const int tile = blockIdx.x * 4 + wave;
  if (tile >= ntn * ntk) return;
  const int n0 = (tile / ntk) * 32, k0 = (tile % ntk) * 64;
  const int64_t m0 = (int64_t)blockIdx.y * kWChunk;
  const int64_t m1 = m0 + kWChunk < M ? m0 + kWChunk : M;
  const int n = n0 + (lane & 31);
  const int ka = k0 + (lane & 31), kb = ka + 32;
  const int hm = lane >> 5;
  f32x16 acc0 = f32x16{}, acc1 = f32x16{};
  double bsum = 0.0;                  // the bias column, in double (one rounding per chunk)
  // uniform trip count for the whole wave (MFMA is a wave-wide instruction); a sample past the
  // chunk end contributes a zero a-operand
  const int pairs = (int)((m1 - m0 + 1) / 2);
  const int64_t mlast = m1 - 1;
  for (int p = 0; p < pairs; ++p) {
    const int64_t m = m0 + 2 * p + hm;
    const int64_t mc = m < mlast ? m : mlast;
    const float av = (n < N && m <= mlast) ? a[mc * lda + n] : 0.0f;
    bsum += (double)av;
    const int64_t xr = x_div == 0 ? 0 : (x_div == 1 ? mc : mc / x_div);
    const float x0 = ka < K ? x[xr * ldx + ka] : (ka == K ? 1.0f : 0.0f);
    const float x1 = kb < K ? x[xr * ldx + kb] : (kb == K ? 1.0f : 0.0f);
    acc0 = mfma32t(av, x0, acc0);
    acc1 = mfma32t(av, x1, acc1);
  }
  float* out = partial + (size_t)blockIdx.y * wgrad_stride(N, K);
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int row = n0 + acc_row(g, hm);
    if (row < N) {
      if (ka < KP) out[(size_t)row * KP + ka] = acc0[g];
      if (kb < KP) out[(size_t)row * KP + kb] = acc1[g];
    }
  }
  // the bias column again from the double sum (the MFMA's f32 value above is overwritten; stores of
  // one wave land in program order)
  bsum += __shfl_xor(bsum, 32);
  if (K >= k0 && K < k0 + 64 && hm == 0 && n < N) out[(size_t)n * KP + K] = (float)bsum;
}

// The main weight-gradient kernel.  A workgroup computes a (64 WN) x (64 WK) output tile of one
// 2048-sample chunk (WN * WK = 4 waves, each owning 64 x 64 = 2 x 2 accumulator tiles of
// v_mfma_f32_32x32x2_f32), streaming the chunk's a and x rows through LDS 16 samples at a time,
// double-buffered: the next stage's 16-byte global loads are in flight while the current
// stage's MFMAs run, one barrier per stage.  Per k-step (two samples) a wave reads 4 operand
// values from LDS for 4 MFMAs; a wave whose n or k range lies past N or K skips its MFMAs.  The
// bias column (sum over samples of a[m][n]) is accumulated from the staged a values by the
// k-tile-0 workgroups on the VALU.  Workgroups sharing a chunk are launched 8 apart so they run
// on the same XCD (blockIdx -> XCD is round-robin) and the chunk's rows come from HBM once per L2.
// Tile shapes: WN=2, WK=2 (128 x 128) for the 256-wide layers; WN=4, WK=1 (256 x 64) when K <= 64.
// Preconditions (host-checked): a, x 16-byte aligned, lda % 4 == 0, ldx % 4 == 0.
constexpr int kWS = 16;        // samples per LDS stage

__device__ __forceinline__ f32x4 load4_masked(const float* __restrict__ p, int valid) {
  if (valid >= 4) return *reinterpret_cast<const f32x4*>(p);
  f32x4 v;
  v[0] = valid > 0 ? p[0] : 0.0f;
  v[1] = valid > 1 ? p[1] : 0.0f;
  v[2] = valid > 2 ? p[2] : 0.0f;
  v[3] = 0.0f;
  return v;
}

// BLK: a in the tile-major row layout (layout.h), and x too when xblk (then x_div == 1); lda / ldx their
// row lengths.
template <int WN, int WK, bool BLK>
__global__ void __launch_bounds__(256, 2)
wgrad_lds_kernel(const float* __restrict__ a, int64_t lda, int N, const float* __restrict__ x, int64_t ldx, int K,
                 int64_t x_div, int xblk, int64_t M, int ntk, int tiles, int chunks, float* __restrict__ partial) {
  static_assert(WN * WK == 4, "four waves");
  constexpr int BN = 64 * WN, BK = 64 * WK;
  constexpr int APAD = BN + 32, XPAD = BK + 32;    // row s+1 lands 32 banks away from row s
  constexpr int AC4 = BN / 4, XC4 = BK / 4;        // float4 columns per staged row
  __shared__ float As[2][kWS][APAD];
  __shared__ float Xs[2][kWS][XPAD];
  __shared__ double bsum[256 / AC4][BN];
  const int b = blockIdx.x;
  const int grp = b / (8 * tiles), rem = b % (8 * tiles);
  const int chunk = grp * 8 + (rem & 7);
  const int tile = rem >> 3;
  if (chunk >= chunks) return;                     // uniform over the block, before any barrier
  const int n0 = (tile / ntk) * BN, k0 = (tile % ntk) * BK;
  const bool do_bias = (tile % ntk) == 0;
  const int64_t m0 = (int64_t)chunk * kWChunk;
  const int64_t m1 = m0 + kWChunk < M ? m0 + kWChunk : M;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wn = w % WN, wk = w / WN;
  // loader: thread tid moves float4 column tid % C4 of rows tid / C4 + (256 / C4) p
  const int a_c = (tid % AC4) * 4, a_r = tid / AC4;
  const int x_c = (tid % XC4) * 4, x_r = tid / XC4;
  constexpr int AROWS = 256 / AC4, XROWS = 256 / XC4;   // rows per pass
  const int a_valid = N - (n0 + a_c), x_valid = K - (k0 + x_c);
  f32x4 ra[WN], rx[WK];
  double bacc[4] = {0.0, 0.0, 0.0, 0.0};      // bias column in double: one rounding per chunk
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  auto load = [&](int64_t mb) __attribute__((always_inline)) {
    static_for<WN>([&](auto pc) __attribute__((always_inline)) {
      constexpr int p = decltype(pc)::value;
      const int64_t m = mb + a_r + AROWS * p;
      const float* ap = BLK ? a + tile_off(m, n0 + a_c, (int)lda) : a + m * lda + n0 + a_c;
      ra[p] = (m < m1 && a_valid > 0) ? load4_masked(ap, a_valid) : zero4;
    });
    static_for<WK>([&](auto pc) __attribute__((always_inline)) {
      constexpr int p = decltype(pc)::value;
      const int64_t m = mb + x_r + XROWS * p;
      const int64_t xr = x_div == 0 ? 0 : (x_div == 1 ? m : m / x_div);
      const float* xp = (BLK && xblk) ? x + tile_off(m, k0 + x_c, (int)ldx) : x + xr * ldx + k0 + x_c;
      rx[p] = (m < m1 && x_valid > 0) ? load4_masked(xp, x_valid) : zero4;
    });
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
    static_for<WN>([&](auto pc) __attribute__((always_inline)) {
      constexpr int p = decltype(pc)::value;
      *reinterpret_cast<f32x4*>(&As[buf][a_r + AROWS * p][a_c]) = ra[p];
      if (do_bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bacc[e] += (double)ra[p][e];
      }
    });
    static_for<WK>([&](auto pc) __attribute__((always_inline)) {
      constexpr int p = decltype(pc)::value;
      *reinterpret_cast<f32x4*>(&Xs[buf][x_r + XROWS * p][x_c]) = rx[p];
    });
  };
  const bool n_act0 = n0 + 64 * wn < N, n_act1 = n0 + 64 * wn + 32 < N;
  const bool k_act0 = k0 + 64 * wk < K, k_act1 = k0 + 64 * wk + 32 < K;
  f32x16 acc00 = f32x16{}, acc01 = f32x16{}, acc10 = f32x16{}, acc11 = f32x16{};
  const int nstages = (int)((m1 - m0 + kWS - 1) / kWS);
  load(m0);
  store(0);
  __syncthreads();
  const int h = lane >> 5, c = lane & 31;
  for (int st = 0; st < nstages; ++st) {
    const int buf = st & 1;
    if (st + 1 < nstages) load(m0 + (int64_t)kWS * (st + 1));
    if (n_act0 && k_act0) {
#pragma unroll
      for (int ks = 0; ks < kWS / 2; ++ks) {
        const float* ar = &As[buf][2 * ks + h][64 * wn + c];
        const float* xr = &Xs[buf][2 * ks + h][64 * wk + c];
        const float a0 = ar[0], a1 = ar[32], x0 = xr[0], x1 = xr[32];
        acc00 = mfma32t(a0, x0, acc00);
        if (k_act1) acc01 = mfma32t(a0, x1, acc01);
        if (n_act1) acc10 = mfma32t(a1, x0, acc10);
        if (n_act1 && k_act1) acc11 = mfma32t(a1, x1, acc11);
      }
    }
    if (st + 1 < nstages) store(buf ^ 1);
    __syncthreads();
  }
  const int KP = K + 1;
  float* out = partial + (size_t)chunk * wgrad_stride(N, K);
  auto emit = [&](const f32x16& acc, int i, int j) __attribute__((always_inline)) {
    const int kk = k0 + 64 * wk + 32 * j + c;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int nn = n0 + 64 * wn + 32 * i + acc_row(g, h);
      if (nn < N && kk < K) out[(size_t)nn * KP + kk] = acc[g];
    }
  };
  emit(acc00, 0, 0);
  emit(acc01, 0, 1);
  emit(acc10, 1, 0);
  emit(acc11, 1, 1);
  if (do_bias) {
    // every staged a row passed through store() exactly once (the prologue stores stage 0)
#pragma unroll
    for (int e = 0; e < 4; ++e) bsum[a_r][a_c + e] = bacc[e];
    __syncthreads();
    if (tid < BN && n0 + tid < N) {
      double sum = 0.0;
#pragma unroll
      for (int r = 0; r < AROWS; ++r) sum += bsum[r][tid];
      out[(size_t)(n0 + tid) * KP + K] = (float)sum;
    }
  }
}

// The bf16x6 weight-gradient kernel of the split MLP arithmetic (nerf_arith F16X3; the GEMMs the
// split-f16 kernels below do not take: in training the per-ray GEMMs over gradient sums, otherwise
// nerf_wgrad's other shapes): the same
// partial sums as wgrad_lds_kernel, on v_mfma_f32_32x32x16_bf16.  Every operand value is split into
// three bf16 parts, x = b0 + b1 + b2 + O(2^-27 x) (each part the RNE bf16 of the f32 remainder, the
// remainders exact), and a k-step accumulates the six products of order >= 2^-16,
//   b0c2 + b1c1 + b2c0 + b0c1 + b1c0 + b0c0   (small terms first; dropped ones O(2^-24)),
// so the result has fp32-level error, at 6 x 32 MFMA cycles per 16 samples against 8 x 64 for
// v_mfma_f32_32x32x2_f32.  bf16 has f32's exponent range: no scaling (gradient rows reach 1e-9).
// A workgroup computes a (64 WN) x (64 WK) tile of one 2048-sample chunk; 16-sample stages are
// split by the loader (a thread owns 8 samples of one column: 8 coalesced dword loads, three
// 16-byte LDS writes) into [part][column][sample] rows of 24 bf16 (48-byte stride: the MFMA
// operand reads, 16 bytes per lane from 16 consecutive rows, are bank-conflict free), double
// buffered with the next stage's loads in flight during the MFMAs.  The bias column sums the
// loader's f32 values.  Workgroups sharing a chunk are launched 8 apart (same XCD).
constexpr int kBfStage = 16;   // samples per stage = one MFMA k-step
constexpr int kBfRow = 24;     // bf16 per LDS row (16 samples + pad)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// The per-stage buffer resources (the 16-sample stage at sample ms: row-major based at row ms and sized
// to the chunk's remaining rows; tile-major based at the stage's place in its 32-sample block, up to the
// block's end, empty past the chunk) are written out in each kernel, not shared: a forceinline
// stage_rsrc<BLK>(base, ld, ms, live, rows_left) moved the compiler's output in every kernel that used
// it (wgrad_bf_kernel, h16_chunk_exps' callers, wgrad_h16w_kernel, wgrad_h16h_kernel,
// wgrad_bf_k64_kernel, wgrad_pair16_kernel: other registers and schedules, up to 33 instructions more),
// also with the row length in bytes passed in.  The same for wgrad_bf_k64_kernel's two-value x split,
// which split3_bf16 (eight values) does not fit.

// v = p0 + p1 + p2 + O(2^-27 v) for 8 values: each part the RNE bf16 of the f32 remainder (exact)
__device__ __forceinline__ void split3_bf16(const float (&v)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h0 = (__bf16)v[j];
    const float r1 = v[j] - (float)h0;
    const __bf16 h1 = (__bf16)r1;
    const float r2 = r1 - (float)h1;
    p0[j] = h0;
    p1[j] = h1;
    p2[j] = (__bf16)r2;
  }
}

__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// XD1 (x_div == 1, one x row per sample: every trunk/head layer): the loader's per-sample offsets
// are stage-invariant VGPRs and only the buffer descriptors move per stage (no VALU address work;
// the generic x path divides and carries per sample, ~130 VALU per stage).
// BLK: a (and x when XD1) tile-major (layout.h): a stage of 16 samples lies in one 32-sample block,
// the stage's resource is based at its first sample's place in that block, a sample j of a slot at
// +32 j bytes; past the chunk end only the sentinel stage (an empty resource) and the zero padding
// of the last block are read.
template <int WN, int WK, bool XD1, bool BLK>
__global__ void __launch_bounds__(256, WN == 4 ? 1 : 2)   // 256 x 64 tiles: 94 KB of LDS, one block per CU
wgrad_bf_kernel(const float* __restrict__ a, int64_t lda, int N, const float* __restrict__ x, int64_t ldx, int K,
                int64_t x_div, int64_t M, int ntk, int tiles, int chunks, int clen, float* __restrict__ partial) {
  static_assert(WN * WK == 4, "four waves");
  constexpr int BN = 64 * WN, BK = 64 * WK;
  constexpr int SA = 2 * BN / 256 > 0 ? 2 * BN / 256 : 1;    // loader slots per thread (column, octet)
  constexpr int SX = 2 * BK / 256 > 0 ? 2 * BK / 256 : 1;
  __shared__ __attribute__((aligned(16))) __bf16 As[2][3][BN][kBfRow];
  __shared__ __attribute__((aligned(16))) __bf16 Xs[2][3][BK][kBfRow];
  __shared__ double bsum[2][BN];
  const int b = blockIdx.x;
  const int grp = b / (8 * tiles), rem = b % (8 * tiles);
  const int chunk = grp * 8 + (rem & 7);
  const int tile = rem >> 3;
  if (chunk >= chunks) return;                     // uniform over the block, before any barrier
  const int n0 = (tile / ntk) * BN, k0 = (tile % ntk) * BK;
  const bool do_bias = (tile % ntk) == 0;
  const int64_t m0 = (int64_t)chunk * clen;
  const int64_t m1 = m0 + clen < M ? m0 + clen : M;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wn = w % WN, wk = w / WN;
  float ra[2][SA][8], rx[2][SX][8];   // two stages in flight: stage k's values in set k % 2
  double bacc[SA];                   // bias column in double: one rounding per chunk
#pragma unroll
  for (int q = 0; q < SA; ++q) bacc[q] = 0.0;
  // Operands through buffer loads (an out-of-range offset reads 0, so no branches in the loader).
  // a: one resource per stage, based at the stage's first row, sized to the chunk's remaining rows;
  // a slot's sample j sits at byte aoff + j*lda4 (past the resource for samples >= m1), and a
  // column >= N gets an offset >= 2^31 (> any resource size: host-checked lda < 2^18).
  // x: based at the chunk's first x row; sample m reads row xrow(m) - xrow(m0) = (r0 + rel) / xd
  // (rel = m - m0, r0 = m0 % xd; xd = 1 per sample, N per ray, "infinite" for one broadcast row),
  // stepped over a slot's 8 samples by a carry instead of a division.
  const uint32_t lda4 = (uint32_t)lda * 4u, ldx4 = (uint32_t)ldx * 4u;
  constexpr uint32_t kOut = 0x80000000u;
  uint32_t aoff[SA], xcol[SX];
#pragma unroll
  for (int q = 0; q < SA; ++q) {
    const int slot = tid + 256 * q, col = slot % BN, oct = slot / BN;
    const int nc = n0 + col;
    aoff[q] = (slot < 2 * BN && nc < N)
                  ? (BLK ? 4u * (uint32_t)(tile_col(nc) + nc % 8 + 64 * oct) : (uint32_t)(8 * oct) * lda4 + 4u * (uint32_t)nc)
                  : kOut;
  }
#pragma unroll
  for (int q = 0; q < SX; ++q) {
    const int slot = tid + 256 * q, col = slot % BK;
    xcol[q] = (slot < 2 * BK && k0 + col < K) ? 4u * (uint32_t)(k0 + col) : kOut;
  }
  uint32_t avo[SA][8], xvo[SX][8];   // XD1: sample j of a slot at a stage-invariant offset
#pragma unroll
  for (int q = 0; q < SA; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) avo[q][j] = aoff[q] == kOut ? kOut : aoff[q] + (uint32_t)j * (BLK ? 32u : lda4);
  if constexpr (XD1) {
#pragma unroll
    for (int q = 0; q < SX; ++q) {
      const int oct = (tid + 256 * q) / BK;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        xvo[q][j] = xcol[q] == kOut ? kOut
                    : BLK ? 4u * (uint32_t)(tile_col(xcol[q] / 4) + (xcol[q] / 4) % 8 + 8 * (8 * oct + j))
                          : (uint32_t)(8 * oct + j) * ldx4 + xcol[q];
    }
  }
  const uint32_t xd = x_div == 0 ? 0xFFFFFFFFu : (uint32_t)x_div;
  const int64_t xr0 = x_div == 0 ? 0 : m0 / x_div;
  const uint32_t r0 = x_div == 0 ? 0u : (uint32_t)(m0 - xr0 * x_div);
  const uint32_t xrows = x_div == 0 ? 1u : (uint32_t)((m1 - 1) / x_div - xr0 + 1);
  const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(x + xr0 * ldx), (short)0, (int)(xrows * ldx4), 0x00020000);
  const uint32_t mrel_end = (uint32_t)(m1 - m0);
  // stage `stage` (< nstages) into register set SET; past the last stage it loads nothing
  auto load = [&](auto set_c, int stage) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    const uint32_t rel0 = (uint32_t)(kBfStage * stage);
    const int64_t ms = m0 + rel0;             // BLK: the stage's place in its block; empty past the chunk
    const bool live = rel0 < mrel_end;
    const __amdgpu_buffer_rsrc_t ares = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(BLK ? a + (ms / 32) * 32 * lda + (ms % 32) * 8 : a + ms * lda), (short)0,
        BLK ? (live ? (int)(32 * lda4 - (ms % 32) * 32) : 0) : (int)((mrel_end - rel0) * lda4), 0x00020000);
#pragma unroll
    for (int q = 0; q < SA; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        ra[SET][q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ares, (int)avo[q][j], 0, kRowLoadAux));
    if constexpr (XD1) {
      const __amdgpu_buffer_rsrc_t xs = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(BLK ? x + (ms / 32) * 32 * ldx + (ms % 32) * 8 : x + ms * ldx), (short)0,
          BLK ? (live ? (int)(32 * ldx4 - (ms % 32) * 32) : 0) : (int)((mrel_end - rel0) * ldx4), 0x00020000);
#pragma unroll
      for (int q = 0; q < SX; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          rx[SET][q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xs, (int)xvo[q][j], 0, kRowLoadAux));
      return;
    }
#pragma unroll
    for (int q = 0; q < SX; ++q) {
      const int slot = tid + 256 * q, oct = slot / BK;
      const uint32_t rel = rel0 + 8u * (uint32_t)oct;
      uint32_t row = (r0 + rel) / xd, r = (r0 + rel) - row * xd;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = rel + j < mrel_end && xcol[q] != kOut;
        const uint32_t off = ok ? row * ldx4 + xcol[q] : kOut;
        rx[SET][q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xres, (int)off, 0, kRowLoadAux));
        if (++r == xd) {
          r = 0;
          ++row;
        }
      }
    }
  };
  auto split_store = [&](float (&v)[8], __bf16 (*dst)[kBfRow], int col, int oct, int plane_stride) {
    bf16x8 p0, p1, p2;
    split3_bf16(v, p0, p1, p2);
    *reinterpret_cast<bf16x8*>(&dst[col][8 * oct]) = p0;
    *reinterpret_cast<bf16x8*>(&dst[col + plane_stride][8 * oct]) = p1;
    *reinterpret_cast<bf16x8*>(&dst[col + 2 * plane_stride][8 * oct]) = p2;
  };
  auto store = [&](auto set_c, int buf) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
#pragma unroll
    for (int q = 0; q < SA; ++q) {
      const int slot = tid + 256 * q, col = slot % BN, oct = slot / BN;
      if (slot < 2 * BN) {
        if (do_bias) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bacc[q] += (double)ra[SET][q][j];
        }
        split_store(ra[SET][q], &As[buf][0][0], col, oct, BN);
      }
    }
#pragma unroll
    for (int q = 0; q < SX; ++q) {
      const int slot = tid + 256 * q, col = slot % BK, oct = slot / BK;
      if (slot < 2 * BK) split_store(rx[SET][q], &Xs[buf][0][0], col, oct, BK);
    }
  };
  const bool n_act0 = n0 + 64 * wn < N, n_act1 = n0 + 64 * wn + 32 < N;
  const bool k_act0 = k0 + 64 * wk < K, k_act1 = k0 + 64 * wk + 32 < K;
  f32x16 acc[2][2] = {{f32x16{}, f32x16{}}, {f32x16{}, f32x16{}}};
  const int nstages = (int)((m1 - m0 + kBfStage - 1) / kBfStage);
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  // Loads run two stages ahead of the MFMAs: iteration st issues stage st+2's loads, splits stage
  // st+1's values (loaded a whole iteration earlier) into the other LDS buffer, and runs stage st's
  // MFMAs.  (One stage ahead, the split waited on loads issued only one MFMA stage before.)
  load(S0{}, 0);
  if (nstages > 1) load(S1{}, 1);
  store(S0{}, 0);
  __syncthreads();
  const int h = lane >> 5, c = lane & 31;
  auto iteration = [&](auto set_c, int st) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;            // st % 2
    using Other = std::integral_constant<int, 1 - SET>;
    const int buf = SET;
    if (st + 2 < nstages) load(set_c, st + 2);
    if (n_act0 && k_act0) {
      bf16x8 fa[2][3], fx[2][3];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[i][p] = *reinterpret_cast<const bf16x8*>(&As[buf][p][64 * wn + 32 * i + c][8 * h]);
          fx[i][p] = *reinterpret_cast<const bf16x8*>(&Xs[buf][p][64 * wk + 32 * i + c][8 * h]);
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if ((i == 1 && !n_act1) || (j == 1 && !k_act1)) continue;
          f32x16 t = acc[i][j];
          t = mfma_bf16(fa[i][0], fx[j][2], t);
          t = mfma_bf16(fa[i][1], fx[j][1], t);
          t = mfma_bf16(fa[i][2], fx[j][0], t);
          t = mfma_bf16(fa[i][0], fx[j][1], t);
          t = mfma_bf16(fa[i][1], fx[j][0], t);
          acc[i][j] = mfma_bf16(fa[i][0], fx[j][0], t);
        }
    }
    if (st + 1 < nstages) store(Other{}, buf ^ 1);
    __syncthreads();
  };
  for (int st = 0; st < nstages; st += 2) {
    iteration(S0{}, st);
    if (st + 1 < nstages) iteration(S1{}, st + 1);
  }
  const int KP = K + 1;
  float* out = partial + (size_t)chunk * wgrad_stride(N, K);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = k0 + 64 * wk + 32 * j + c;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int nn = n0 + 64 * wn + 32 * i + acc_row(g, h);
        if (nn < N && kk < K) out[(size_t)nn * KP + kk] = acc[i][j][g];
      }
    }
  if (do_bias) {
    // every staged a value passed through store() exactly once (the prologue stores stage 0)
#pragma unroll
    for (int q = 0; q < SA; ++q) {
      const int slot = tid + 256 * q, col = slot % BN, oct = slot / BN;
      if (slot < 2 * BN) bsum[oct][col] = bacc[q];
    }
    __syncthreads();
    if (tid < BN && n0 + tid < N) out[(size_t)(n0 + tid) * KP + K] = (float)(bsum[0][tid] + bsum[1][tid]);
  }
}

// The whole-tile (256 x 256) weight gradients: the trunk layers' d pre_l over h_{l-1}, the skip
// layer's h3 block and dir/density over h7.
constexpr int kWT = 256;
// ------------------------------------------------- split-f16 ("f16x3") weight gradient, 256 columns
// The whole-tile GEMM (a chunk's 256 x 256 weight gradient in one workgroup) on
// v_mfma_f32_32x32x16_f16 with three products per fp32 product instead of bf16x6's six: every operand value is split as v s = hi + lo (f16 each, lo =
// f16(v s - hi), the residual exact in f32) and a k-step accumulates lo(a)hi(x) + hi(a)lo(x) +
// hi(a)hi(x) (small terms first; the dropped lo lo term and the split residual are O(2^-22) of the
// product), half the MFMAs and two thirds of the split VALU of bf16x6.  f16 lacks f32's exponent
// range, so each operand carries one power-of-two scale per chunk, s = 2^(14 - e) with e the
// exponent of the chunk's largest |value| (every v s < 2^14: no f16 overflow).  The MFMAs accumulate
// in place (AGPRs) at those scales and the partial is unscaled once at the store (exact: powers of
// two).  A value far below its chunk's maximum keeps an absolute error <= 2^-25 / s = 2^-39 of that
// maximum, far below an fp32 sum's rounding of the terms near it.
// The chunk maxima come from the producers: the f16x3 forward and data-gradient kernels record each
// 32-sample block's exponent per operand slice (layout.h, block exponents); the kernel takes the
// largest over its chunk's blocks.  Without records (rows from another writer) it first reads the
// chunk once to find them (workgroup-uniform branch before the GEMM).
constexpr int kH16EMin = -100;        // scale floor exponent (an all-zero or tiny chunk)

// v s = hi + lo for 8 values at scale s (hi by v_cvt_pk_f16_f32, lo by split_lo_pair)
__device__ __forceinline__ void split2_f16(const float (&v)[8], float s, h16x8& hi, h16x8& lo) {
  typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = v[2 * p] * s, x1 = v[2 * p + 1] * s;
    const h16x2 hi2 = {(_Float16)x0, (_Float16)x1};
    const h16x2 lo2 = __builtin_bit_cast(h16x2, split_lo_pair(__builtin_bit_cast(uint32_t, hi2), x0, x1));
    hi[2 * p] = hi2[0];
    hi[2 * p + 1] = hi2[1];
    lo[2 * p] = lo2[0];
    lo[2 * p + 1] = lo2[1];
  }
}

// The chunk's exponents (Ea, Ex; wave-uniform, the same in every wave of the workgroup) for the
// split-f16 whole-tile GEMMs: from the block records (lanes 0..31: one block each), else by a pass
// over the chunk's whole 32-sample blocks (the records' span: a chunk shorter than a block gets the
// exponents the records would give it; a: column tid of the staged rows, counting meta.a_cols of
// them; x: the wave's fragment columns).  wmax: 8 floats of LDS.
template <bool BLK>
__device__ __forceinline__ void h16_chunk_exps(const float* __restrict__ a, int64_t lda, const float* __restrict__ x,
                                               int64_t ldx, int64_t M, int64_t m0, int64_t m1, const H16Meta& meta,
                                               float (&wmax)[4][2], int& Ea, int& Ex) {
  const int tid = threadIdx.x, lane = tid & 63, wk = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  const int64_t b0 = m0 / 32, nb = (m1 - 1) / 32 - b0 + 1;   // blocks of the chunk (<= 64)
  float ra_rec = 0.0f, rx_rec = 0.0f, bad = 0.0f;            // 1000 + e of the lane's blocks; 1: a record absent
  if (meta.a && meta.x) {
    for (int64_t b = lane; b < nb; b += 64) {
      const float va = meta.a[(b0 + b) * meta.a_stride], vx = meta.x[(b0 + b) * meta.x_stride];
      bad = (block_exp_valid(va) && block_exp_valid(vx)) ? bad : 1.0f;
      ra_rec = fmaxf(ra_rec, -va);
      rx_rec = fmaxf(rx_rec, -vx);
    }
  }
  const bool have = meta.a && meta.x && wave_max_nn(bad) == 0.0f;   // uniform (every wave alike)
  if (have) {
    Ea = (int)wave_max_nn(ra_rec) - kBlockExpBias;
    Ex = (int)wave_max_nn(rx_rec) - kBlockExpBias;
  } else {
    const uint32_t lda4 = (uint32_t)lda * 4u, ldx4 = (uint32_t)ldx * 4u;
    const uint32_t avo = BLK ? 4u * (uint32_t)(tile_col(tid) + tid % 8) : 4u * (uint32_t)tid;
    const uint32_t as4 = BLK ? 32u : lda4, xs4 = BLK ? 32u : ldx4;
    uint32_t xvo[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int xc = 64 * wk + 32 * t + c;
      xvo[t] = BLK ? 4u * (uint32_t)(tile_col(xc) + xc % 8 + 64 * h) : (uint32_t)(8 * h) * ldx4 + 4u * (uint32_t)xc;
    }
    float ma = 0.0f, mx = 0.0f;
    const int64_t f0 = b0 * 32, f1 = (b0 + nb) * 32 < M ? (b0 + nb) * 32 : M;
    for (int64_t ms = f0; ms < f1; ms += kBfStage) {
      const uint32_t left = (uint32_t)(f1 - ms);
      const __amdgpu_buffer_rsrc_t ares = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(BLK ? a + (ms / 32) * 32 * lda + (ms % 32) * 8 : a + ms * lda), (short)0,
          BLK ? (int)(32 * lda4 - (ms % 32) * 32) : (int)((left < kBfStage ? left : kBfStage) * lda4), 0x00020000);
      const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(BLK ? x + (ms / 32) * 32 * ldx + (ms % 32) * 8 : x + ms * ldx), (short)0,
          BLK ? (int)(32 * ldx4 - (ms % 32) * 32) : (int)((left < kBfStage ? left : kBfStage) * ldx4), 0x00020000);
#pragma unroll
      for (int j = 0; j < 16; ++j)
        ma = fmaxf(ma, fabsf(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ares, (int)avo, (int)(j * as4), 0))));
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          mx = fmaxf(mx, fabsf(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xres, (int)xvo[t], (int)(j * xs4), 0))));
    }
    ma = wave_max_nn(tid < meta.a_cols ? ma : 0.0f);
    mx = wave_max_nn(mx);
    wmax[wk][0] = ma;                // (every lane the same value)
    wmax[wk][1] = mx;
    __syncthreads();
    ma = fmaxf(fmaxf(wmax[0][0], wmax[1][0]), fmaxf(wmax[2][0], wmax[3][0]));
    mx = fmaxf(fmaxf(wmax[0][1], wmax[1][1]), fmaxf(wmax[2][1], wmax[3][1]));
    Ea = (int)(-block_exp_record(ma)) - kBlockExpBias;
    Ex = (int)(-block_exp_record(mx)) - kBlockExpBias;
  }
  Ea = __builtin_amdgcn_readfirstlane(Ea < kH16EMin ? kH16EMin : Ea);
  Ex = __builtin_amdgcn_readfirstlane(Ex < kH16EMin ? kH16EMin : Ex);
}

typedef _Float16 H16Stage[2][2][kWT][kBfRow];   // [buffer][hi, lo][column][sample]
// (row-major rows: nerf_wgrad's operands; the tile-major training path runs wgrad_h16h_kernel)
__device__ __forceinline__ void h16w_chunk(const float* __restrict__ a, int64_t lda, const float* __restrict__ x,
                                           int64_t ldx, int64_t M, int clen, const H16Meta& meta,
                                           float* __restrict__ partial, int chunk, H16Stage& As, float (&wmax)[4][2]) {
  const int64_t m0 = (int64_t)chunk * clen;
  const int64_t m1 = m0 + clen < M ? m0 + clen : M;
  const int tid = threadIdx.x, lane = tid & 63, wk = tid >> 6;   // wave wk: columns 64 wk ..
  const int h = lane >> 5, c = lane & 31;
  const uint32_t lda4 = (uint32_t)lda * 4u, ldx4 = (uint32_t)ldx * 4u;
  // (tid < kWT always; the comparison here and at the bias store is kept from the version with fewer
  // row tiles so that the kernel's instruction list stays as it was)
  const uint32_t avo = tid >= kWT ? 0x80000000u : 4u * (uint32_t)tid;
  uint32_t xvo[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int xc = 64 * wk + 32 * t + c;
    xvo[t] = (uint32_t)(8 * h) * ldx4 + 4u * (uint32_t)xc;
  }
  const uint32_t mrel_end = (uint32_t)(m1 - m0);
  float ra[4][16], rx[4][2][8];
  double bacc = 0.0;
  auto load = [&](auto set_c, int stage) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    const uint32_t rel0 = (uint32_t)(kBfStage * stage) < mrel_end ? (uint32_t)(kBfStage * stage) : mrel_end;
    const int64_t ms = m0 + rel0;
    const __amdgpu_buffer_rsrc_t ares = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a + ms * lda), (short)0, (int)((mrel_end - rel0) * lda4), 0x00020000);
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(x + ms * ldx), (short)0, (int)((mrel_end - rel0) * ldx4), 0x00020000);
#pragma unroll
    for (int j = 0; j < 16; ++j)
      ra[SET][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ares, (int)avo, (int)(j * lda4), kRowLoadAux));
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        rx[SET][t][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xres, (int)xvo[t], (int)(j * ldx4), kRowLoadAux));
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  using C2 = std::integral_constant<int, 2>;

  // ---- the chunk's exponents (records, else a pass over the chunk)
  int Ea, Ex;
  h16_chunk_exps<false>(a, lda, x, ldx, M, m0, m1, meta, wmax, Ea, Ex);
  const float sa = ldexpf(1.0f, 14 - Ea), sx = ldexpf(1.0f, 14 - Ex);

  h16x8 fx[2][2][2];                   // split x fragments of stages st (fx[st & 1]) and st+1: [t][hi, lo]
  auto split_x = [&](auto set_c, auto fb_c) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value, FB = decltype(fb_c)::value;
#pragma unroll
    for (int t = 0; t < 2; ++t) split2_f16(rx[SET][t], sx, fx[FB][t][0], fx[FB][t][1]);
  };
  auto split_a = [&](auto set_c, int buf) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
#pragma unroll
    for (int j = 0; j < 16; ++j) bacc += (double)ra[SET][j];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = ra[SET][8 * o + j];
      h16x8 hi, lo;
      split2_f16(v, sa, hi, lo);
      *reinterpret_cast<h16x8*>(&As[buf][0][tid][8 * o]) = hi;
      *reinterpret_cast<h16x8*>(&As[buf][1][tid][8 * o]) = lo;
    }
  };
  f32x16 acc[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i][0] = acc[i][1] = f32x16{};
  const int nstages = (int)((mrel_end + 4 * kBfStage - 1) / (4 * kBfStage)) * 4;
  load(C0{}, 0);
  load(C1{}, 1);
  load(C2{}, 2);
  split_x(C0{}, C0{});
  split_a(C0{}, 0);
  __syncthreads();
  // iteration st (set st % 4, buffers st % 2): stage st+3's loads; stage st's MFMAs with stage st+1's
  // splits in their shadow; barrier
  auto iteration = [&](auto set_c, int st) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value, FB = SET & 1;
    using Nxt = std::integral_constant<int, (SET + 1) & 3>;
    using Ld = std::integral_constant<int, (SET + 3) & 3>;
    using FBn = std::integral_constant<int, FB ^ 1>;
    load(Ld{}, st + 3);
    __builtin_amdgcn_sched_barrier(0);
    h16x8 fa[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p) fa[0][p] = *reinterpret_cast<const h16x8*>(&As[FB][p][c][8 * h]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i + 1 < 8) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
          fa[(i + 1) & 1][p] = *reinterpret_cast<const h16x8*>(&As[FB][p][32 * (i + 1) + c][8 * h]);
      }
      const h16x8 (&f)[2] = fa[i & 1];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x16 t = acc[i][j];
        t = mfma16(f[1], fx[FB][j][0], t);
        t = mfma16(f[0], fx[FB][j][1], t);
        acc[i][j] = mfma16(f[0], fx[FB][j][0], t);
      }
    }
    split_x(Nxt{}, FBn{});
    split_a(Nxt{}, FB ^ 1);
    // schedule: per row tile 2 fragment reads (the next tile's), then its 6 MFMAs each followed by
    // VALU of the next stage's splits; the split's LDS writes last
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);         // tile 0's reads
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i + 1 < 8) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);   // DS reads (tile i+1)
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);     // MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);         // VALU
      }
    }
    __builtin_amdgcn_sched_group_barrier(0x200, 4, 0);         // DS writes
    __syncthreads();
  };
  for (int st = 0; st < nstages; st += 4) {
    iteration(C0{}, st);
    iteration(C1{}, st + 1);
    iteration(C2{}, st + 2);
    iteration(std::integral_constant<int, 3>{}, st + 3);
  }
  // the partial at the chunk's scales; its exponent eo (true = stored 2^eo) in the partial's trailing
  // slot, applied by the reduction (a VALU unscale here would pull the accumulators out of the AGPRs)
  constexpr int KP = kWT + 1;
  const int64_t stride = wgrad_stride(kWT, kWT);
  float* out = partial + (size_t)chunk * stride;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = 64 * wk + 32 * j + c;
#pragma unroll
      for (int g = 0; g < 16; ++g) out[(size_t)(32 * i + acc_row(g, h)) * KP + kk] = acc[i][j][g];
    }
  if (tid < kWT) out[(size_t)tid * KP + kWT] = (float)bacc;   // (the bias column: unscaled)
  if (tid == 0) reinterpret_cast<int*>(out)[stride - 4] = Ea + Ex - 28;   // acc = sum (a 2^(14-Ea)) (x 2^(14-Ex))
}

__global__ void __launch_bounds__(256, 1)
wgrad_h16w_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ x, int64_t ldx, int64_t M,
                  int clen, H16Meta meta, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) H16Stage As;
  __shared__ float wmax[4][2];
  h16w_chunk(a, lda, x, ldx, M, clen, meta, partial, blockIdx.x, As, wmax);
}

// The same 256 x 256 GEMM (tile-major rows) with two workgroups per CU: each workgroup computes half
// the output rows (a columns 128 half .. +127: 4 row tiles x 2 column tiles per wave, 128 accumulators)
// so the two workgroups' waves (two per SIMD) fill each other's load, split and barrier waits, which a
// lone workgroup per CU runs in lock-step ("What bounds the phase now").  Both halves read
// all of x: block b runs chunk (b / 16) 8 + b % 8, half (b / 8) % 2, so the halves of a chunk sit on
// one XCD (b and b + 8) and the second read of x hits its L2.  Three raw-load sets: loads run two
// stages ahead; the x split runs just before its stage's MFMAs (one fragment set, not two).
// nrows < 256 (the dir/density launch: 160): a columns from nrows on are not read (zeros) and
// output rows from nrows on are not stored; the partial has nrows rows (wgrad_stride(nrows, 256)).
// The bias column: each a column has two threads (samples 0-7 and 8-15 of every stage), each summing
// in double; their sums are added once at the end (wgrad_h16w_kernel: one thread, all 16).
// SUMS (the dir/density launch, rays of N % 32 == 0 samples): the threads of a columns 0..127
// (d pre_dir) also write each stage's sum of their 8 raw values (in double, rounded once) to
// sums[(m / 8) * 128 + column], m the first of the 8 samples: the per-ray inputs' GEMMs (dir_linear's
// PE_4(d) columns) then run over M / 8 rows of these sums instead of re-reading the gradient rows
// (ray_sums_kernel's 256 columns per sample).
template <bool SUMS>
__global__ void __launch_bounds__(256, 2)
wgrad_h16h_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ x, int64_t ldx, int64_t M,
                  int clen, int chunks, int nrows, H16Meta meta, float* __restrict__ partial,
                  float* __restrict__ sums) {
  __shared__ __attribute__((aligned(16))) _Float16 As[2][2][128][kBfRow];   // [buffer][hi, lo][column][sample]
  __shared__ float wmax[4][2];
  __shared__ double bsum[128];
  const int b = blockIdx.x;
  const int chunk = (b >> 4) * 8 + (b & 7), half = (b >> 3) & 1;
  if (chunk >= chunks) return;
  const int64_t m0 = (int64_t)chunk * clen;
  const int64_t m1 = m0 + clen < M ? m0 + clen : M;
  const int tid = threadIdx.x, lane = tid & 63, wk = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  const uint32_t lda4 = (uint32_t)lda * 4u, ldx4 = (uint32_t)ldx * 4u;
  const int ac = 128 * half + (tid & 127), as0 = 8 * (tid >> 7);   // the thread's a column, its first sample
  // a columns past the kept rows' whole feature groups (meta.a_cols; the dir/density launch: 129 of 160
  // -> 136) are not read: their rows are dropped, and an offset beyond the resource reads 0
  const int acols = (meta.a_cols + 7) / 8 * 8 < nrows ? (meta.a_cols + 7) / 8 * 8 : nrows;
  const uint32_t avo = ac < acols ? 4u * (uint32_t)(tile_col(ac) + ac % 8) + 32u * (uint32_t)as0 : 0x80000000u;
  uint32_t xvo[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int xc = 64 * wk + 32 * t + c;
    xvo[t] = 4u * (uint32_t)(tile_col(xc) + xc % 8 + 64 * h);
  }
  const uint32_t mrel_end = (uint32_t)(m1 - m0);
  float ra[3][8], rx[3][2][8];
  double bacc = 0.0;
  auto load = [&](auto set_c, int stage) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    const uint32_t rel0 = (uint32_t)(kBfStage * stage) < mrel_end ? (uint32_t)(kBfStage * stage) : mrel_end;
    const int64_t ms = m0 + rel0;
    const bool live = rel0 < mrel_end;
    const __amdgpu_buffer_rsrc_t ares = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a + (ms / 32) * 32 * lda + (ms % 32) * 8), (short)0,
        live ? (int)(32 * lda4 - (ms % 32) * 32) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(x + (ms / 32) * 32 * ldx + (ms % 32) * 8), (short)0,
        live ? (int)(32 * ldx4 - (ms % 32) * 32) : 0, 0x00020000);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      ra[SET][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ares, (int)avo, j * 32, kRowLoadAux));
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        rx[SET][t][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xres, (int)xvo[t], j * 32, kRowLoadAux));
  };
  int Ea, Ex;
  h16_chunk_exps<true>(a, lda, x, ldx, M, m0, m1, meta, wmax, Ea, Ex);
  const float sa = ldexpf(1.0f, 14 - Ea), sx = ldexpf(1.0f, 14 - Ex);
  __amdgpu_buffer_rsrc_t sres;   // SUMS: this chunk's rows of 8-sample sums (half 0 only)
  if constexpr (SUMS)
    sres = __builtin_amdgcn_make_buffer_rsrc(sums + (m0 / 8) * kDirHidden, (short)0,
                                             half == 0 ? (int)(mrel_end / 8 * kDirHidden * 4) : 0, 0x00020000);
  auto split_a = [&](auto set_c, int buf, int stage) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    double ps = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) ps += (double)ra[SET][j];
    bacc += ps;
    // float (m0 + 16 stage + as0) / 8 * 128 + (tid & 127) = (m0 / 8 + 2 stage) 128 + tid; past the
    // chunk (and in the half-1 workgroups) the store falls outside the resource and is dropped
    if constexpr (SUMS)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((float)ps), sres, 4 * tid, 2 * kDirHidden * 4 * stage,
                                            kRowStoreAux);
    h16x8 hi, lo;
    split2_f16(ra[SET], sa, hi, lo);
    *reinterpret_cast<h16x8*>(&As[buf][0][tid & 127][as0]) = hi;
    *reinterpret_cast<h16x8*>(&As[buf][1][tid & 127][as0]) = lo;
  };
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x16{};
  // six iterations per loop trip (3 load sets x 2 LDS buffers); the extra stages add zeros
  const int nstages = (int)((mrel_end + 6 * kBfStage - 1) / (6 * kBfStage)) * 6;
  load(std::integral_constant<int, 0>{}, 0);
  load(std::integral_constant<int, 1>{}, 1);
  split_a(std::integral_constant<int, 0>{}, 0, 0);
  __syncthreads();
  // iteration st (IT = st mod 6: set IT % 3, buffer IT % 2): stage st+2's loads; stage st's x
  // split and MFMAs, stage st+1's a split in their shadow; barrier
  auto iteration = [&](auto it_c, int st) __attribute__((always_inline)) {
    constexpr int IT = decltype(it_c)::value, SET = IT % 3, FB = IT & 1;
    using Nxt = std::integral_constant<int, (IT + 1) % 3>;
    using Ld = std::integral_constant<int, (IT + 2) % 3>;
    load(Ld{}, st + 2);
    __builtin_amdgcn_sched_barrier(0);
    h16x8 fx[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) split2_f16(rx[SET][t], sx, fx[t][0], fx[t][1]);
    h16x8 fa[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p) fa[0][p] = *reinterpret_cast<const h16x8*>(&As[FB][p][c][8 * h]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i + 1 < 4) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
          fa[(i + 1) & 1][p] = *reinterpret_cast<const h16x8*>(&As[FB][p][32 * (i + 1) + c][8 * h]);
      }
      const h16x8 (&f)[2] = fa[i & 1];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x16 t = acc[i][j];
        t = mfma16(f[1], fx[j][0], t);
        t = mfma16(f[0], fx[j][1], t);
        acc[i][j] = mfma16(f[0], fx[j][0], t);
      }
    }
    split_a(Nxt{}, FB ^ 1, st + 1);
    __builtin_amdgcn_sched_group_barrier(0x002, 40, 0);        // the x split
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);         // tile 0's reads
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i + 1 < 4) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      }
    }
    __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
    __syncthreads();
  };
  for (int st = 0; st < nstages; st += 6) {
    iteration(std::integral_constant<int, 0>{}, st);
    iteration(std::integral_constant<int, 1>{}, st + 1);
    iteration(std::integral_constant<int, 2>{}, st + 2);
    iteration(std::integral_constant<int, 3>{}, st + 3);
    iteration(std::integral_constant<int, 4>{}, st + 4);
    iteration(std::integral_constant<int, 5>{}, st + 5);
  }
  constexpr int KP = kWT + 1;
  const int64_t stride = wgrad_stride(nrows, kWT);
  float* out = partial + (size_t)chunk * stride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (128 * half + 32 * i < nrows) {   // (uniform: whole row tiles past the kept rows are dropped)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int kk = 64 * wk + 32 * j + c;
#pragma unroll
        for (int g = 0; g < 16; ++g)
          out[(size_t)(128 * half + 32 * i + acc_row(g, h)) * KP + kk] = acc[i][j][g];
      }
    }
  }
  if (tid >= 128) bsum[tid - 128] = bacc;   // samples 8..15 of each stage
  __syncthreads();
  if (tid < 128 && ac < nrows) out[(size_t)ac * KP + kWT] = (float)(bacc + bsum[tid]);
  if (tid == 0 && half == 0) reinterpret_cast<int*>(out)[stride - 4] = Ea + Ex - 28;
}

// 256 x (K <= 64) weight gradients with one x row per sample (layer 0 and the skip layer's PE
// columns): 8 waves, wave w owns output rows 32w .. 32w+31 (one MFMA row tile, two column tiles).
// Each wave loads its own a columns straight in A-fragment order (lane (c, h): column 32w + c,
// samples 8h .. 8h+7) and splits them in registers; x (64 columns, shared by all waves) is split
// once per workgroup into LDS (each thread: one column, two samples).  Little LDS and few
// registers, so two workgroups share a CU and keep more loads in flight (1 KiB of a + 252 B of x
// per sample).  Loads run two stages ahead, unconditionally.  75 us per 262K-sample launch against
// 105 us on 256 x 64 tiles of wgrad_bf_kernel (scripts/wgrad_libs_trace.sh, K=63).
// (The split arithmetic's layer-0 / skip-PE pair runs wgrad_pair16_kernel below: this kernel serves
// nerf_wgrad's 256 x (K <= 64) GEMMs under f16x3.)
template <bool BLK>   // BLK: a and x tile-major (layout.h; see wgrad_bf_kernel)
__global__ void __launch_bounds__(512)
wgrad_bf_k64_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ x, int64_t ldx, int K,
                    int64_t M, int clen, float* __restrict__ partial) {
  constexpr int XS = 2;              // x samples per thread and stage (16 over the 8 waves)
  __shared__ __attribute__((aligned(16))) __bf16 Xs[2][3][64][kBfRow];
  const int chunk = blockIdx.x;
  const int64_t m0 = (int64_t)chunk * clen;
  const int64_t m1 = m0 + clen < M ? m0 + clen : M;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, c = lane & 31;
  const uint32_t lda4 = (uint32_t)lda * 4u, ldx4 = (uint32_t)ldx * 4u;
  const int ac = 32 * (w & 7) + c;
  const uint32_t avo = BLK ? 4u * (uint32_t)(tile_col(ac) + ac % 8 + 64 * h) : (uint32_t)(8 * h) * lda4 + 4u * (uint32_t)ac;
  const uint32_t as4 = BLK ? 32u : lda4, xs4 = BLK ? 32u : ldx4;   // byte step from sample j to j + 1
  // x loader: column tid % 64 (past K: an offset beyond any resource, reads 0), samples XS p .. + XS-1
  const int xc = tid & 63, xp = tid >> 6;
  const uint32_t xvo = xc < K ? (BLK ? 4u * (uint32_t)(tile_col(xc) + xc % 8 + 8 * XS * xp)
                                     : (uint32_t)(XS * xp) * ldx4 + 4u * (uint32_t)xc)
                              : 0x80000000u;
  const uint32_t mrel_end = (uint32_t)(m1 - m0);
  float ra[2][8], rx[2][XS];
  double bacc = 0.0;                 // bias column in double: one rounding per chunk
  auto load = [&](auto set_c, int stage) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    const uint32_t rel0 = (uint32_t)(kBfStage * stage) < mrel_end ? (uint32_t)(kBfStage * stage) : mrel_end;
    const int64_t ms = m0 + rel0;
    const bool live = rel0 < mrel_end;
    const __amdgpu_buffer_rsrc_t ares = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(BLK ? a + (ms / 32) * 32 * lda + (ms % 32) * 8 : a + ms * lda), (short)0,
        BLK ? (live ? (int)(32 * lda4 - (ms % 32) * 32) : 0) : (int)((mrel_end - rel0) * lda4), 0x00020000);
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(BLK ? x + (ms / 32) * 32 * ldx + (ms % 32) * 8 : x + ms * ldx), (short)0,
        BLK ? (live ? (int)(32 * ldx4 - (ms % 32) * 32) : 0) : (int)((mrel_end - rel0) * ldx4), 0x00020000);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      ra[SET][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ares, (int)avo, (int)(j * as4), kRowLoadAux));
#pragma unroll
    for (int j = 0; j < XS; ++j)
      rx[SET][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xres, (int)xvo, (int)(j * xs4), kRowLoadAux));
  };
  auto store_x = [&](auto set_c, int buf) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    // (two values per thread: split3_bf16 takes eight, so the split is written out here)
    __bf16 p[3][XS];
#pragma unroll
    for (int j = 0; j < XS; ++j) {
      const float v = rx[SET][j];
      const __bf16 h0 = (__bf16)v;
      const float r1 = v - (float)h0;
      const __bf16 h1 = (__bf16)r1;
      p[0][j] = h0;
      p[1][j] = h1;
      p[2][j] = (__bf16)(r1 - (float)h1);
    }
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int q = 0; q < 3; ++q) *reinterpret_cast<bf16x2*>(&Xs[buf][q][xc][2 * xp]) = bf16x2{p[q][0], p[q][1]};
  };
  f32x16 acc[2] = {f32x16{}, f32x16{}};
  const int nstages = (int)((m1 - m0 + 2 * kBfStage - 1) / (2 * kBfStage)) * 2;   // even; the extra reads zeros
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  load(S0{}, 0);
  load(S1{}, 1);
  store_x(S0{}, 0);
  __syncthreads();
  // iteration st: split stage st's a (set st % 2) into fragments, reuse the set for stage st+2,
  // stage st's MFMAs (x from LDS buffer st % 2), stage st+1's x into the other buffer
  auto iteration = [&](auto set_c, int st) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    using Other = std::integral_constant<int, 1 - SET>;
    const int buf = SET;
    bf16x8 fa[3];
#pragma unroll
    for (int j = 0; j < 8; ++j) bacc += (double)ra[SET][j];
    split3_bf16(ra[SET], fa[0], fa[1], fa[2]);
    load(set_c, st + 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      bf16x8 fx[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) fx[q] = *reinterpret_cast<const bf16x8*>(&Xs[buf][q][32 * t + c][8 * h]);
      f32x16 v = acc[t];
      v = mfma_bf16(fa[0], fx[2], v);
      v = mfma_bf16(fa[1], fx[1], v);
      v = mfma_bf16(fa[2], fx[0], v);
      v = mfma_bf16(fa[0], fx[1], v);
      v = mfma_bf16(fa[1], fx[0], v);
      acc[t] = mfma_bf16(fa[0], fx[0], v);
    }
    store_x(Other{}, buf ^ 1);   // (after the last stage: zeros into the idle buffer)
    __syncthreads();
  };
  for (int st = 0; st < nstages; st += 2) {
    iteration(S0{}, st);
    iteration(S1{}, st + 1);
  }
  const int KP = K + 1;
  float* out = partial + (size_t)chunk * wgrad_stride(kWT, K);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int kk = 32 * t + c;
    if (kk < K) {
#pragma unroll
      for (int g = 0; g < 16; ++g) out[(size_t)(32 * w + acc_row(g, h)) * KP + kk] = acc[t][g];
    }
  }
  // bias column: this lane summed column 32w + c over its 8 samples of every stage
  bacc += __shfl_xor(bacc, 32);
  if (h == 0) out[(size_t)(32 * w + c) * KP + K] = (float)bacc;
}

// Layer 0's weight gradient (d pre_0 over enc_x) and the skip layer's PE columns (d pre_4 over enc_x)
// of the split arithmetic as one 512 x 63 GEMM on split-f16 MFMA (wgrad_bf_k64_kernel<true>'s
// shape with wgrad_h16h_kernel's arithmetic: three f16 products per fp32 product instead of bf16x6's
// six, two f16 parts to split instead of three bf16 parts).  16 waves per chunk (kPairClen): wave w
// owns output rows 32w .. 32w+31 (waves 0-7 of d pre_0, 8-15 of d pre_4; one MFMA row tile, two
// column tiles), loads its a columns straight in A-fragment order and splits them in registers; x =
// enc_x (63 columns + the pad slot, which is never read) is split once per workgroup into LDS, one
// sample of one column per thread and stage.  enc_x is read once for both gradients.
// Scales: one power of two per chunk and operand, s = 2^(14 - e) (h16_chunk_exps), from the producers'
// block exponent records (layout.h: d pre_0 = gradient entry 8, d pre_4 = entry 3, enc_x = save entry
// 8), else from a pass over the chunk (workgroup-uniform branch).  The two halves' a scales differ, so
// each wave unscales its 32 accumulators itself (exact: powers of two) and the partial is plain fp32
// (wgrad_reduce_kernel, scaled = 0).  The bias column sums the raw a values in double.
// 274 us per step beside the other stream against 298 us for the bf16x6 kernel it replaced; a variant
// without LDS or barriers (every wave loading and splitting all 64 enc_x columns itself) took 372 us:
// the 16 waves' dword gathers of x cost more than the per-stage barrier (profiles/r06/
// kernel_stats_train_a.csv, kernel_stats_train_b.csv).
constexpr int kPairWaves = 16;
__global__ void __launch_bounds__(64 * kPairWaves)
wgrad_pair16_kernel(const float* __restrict__ grad, const float* __restrict__ save, int64_t M, int clen,
                    float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) _Float16 Xs[2][2][64][kBfRow];   // [buffer][hi, lo][column][sample]
  __shared__ float wmax[kPairWaves][2];
  const int chunk = blockIdx.x;
  const int64_t m0 = (int64_t)chunk * clen;
  const int64_t m1 = m0 + clen < M ? m0 + clen : M;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = lane >> 5, c = lane & 31, half = w >> 3;
  const float* a = grad + tile_col(half ? kSkipLayer * kHidden : 0);     // (wave-uniform)
  const float* x = save + tile_col(kSaveEncX);
  constexpr uint32_t lda4 = kGradRow * 4u, ldx4 = kSaveRow * 4u;
  const int ac = 32 * (w & 7) + c;
  const uint32_t avo = 4u * (uint32_t)(tile_col(ac) + ac % 8 + 64 * h);   // sample j of the stage at + 32 j bytes
  const int xc = tid & 63, xp = tid >> 6;                                 // x: column xc, sample xp of a stage
  const uint32_t xvo = xc < kPosEnc ? 4u * (uint32_t)(tile_col(xc) + xc % 8 + 8 * xp) : 0x80000000u;
  const uint32_t mrel_end = (uint32_t)(m1 - m0);

  // ---- the chunk's exponents: records (every wave reads all three, so the branch is uniform)
  const int64_t b0 = m0 / 32, nb = (m1 - 1) / 32 - b0 + 1;
  const float* rec0 = grad + tile_col(kMetaGradF) + kMetaGradF % 8 + 8 * 8;   // entry 8: d pre_0
  const float* rec4 = grad + tile_col(kMetaGradF) + kMetaGradF % 8 + 8 * 3;   // entry 3: d pre_4
  const float* recx = save + tile_col(kMetaSaveF) + kMetaSaveF % 8 + 8 * 8;   // entry 8: enc_x
  float r0 = 0.0f, r4 = 0.0f, rx_ = 0.0f, bad = 0.0f;
  for (int64_t b = lane; b < nb; b += 64) {
    const float v0 = rec0[(b0 + b) * 32 * kGradRow], v4 = rec4[(b0 + b) * 32 * kGradRow];
    const float vx = recx[(b0 + b) * 32 * kSaveRow];
    bad = (block_exp_valid(v0) && block_exp_valid(v4) && block_exp_valid(vx)) ? bad : 1.0f;
    r0 = fmaxf(r0, -v0);
    r4 = fmaxf(r4, -v4);
    rx_ = fmaxf(rx_, -vx);
  }
  int Ea, Ex;
  if (wave_max_nn(bad) == 0.0f) {
    Ea = (int)wave_max_nn(half ? r4 : r0) - kBlockExpBias;
    Ex = (int)wave_max_nn(rx_) - kBlockExpBias;
  } else {   // absent: the chunk's whole 32-sample blocks read once (the records' span)
    float ma = 0.0f, mx = 0.0f;
    const int64_t f0 = b0 * 32, f1 = (b0 + nb) * 32 < M ? (b0 + nb) * 32 : M;
    for (int64_t ms = f0; ms < f1; ms += kBfStage) {
      const __amdgpu_buffer_rsrc_t ares = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(a + (ms / 32) * 32 * kGradRow + (ms % 32) * 8), (short)0, (int)(32 * lda4 - (ms % 32) * 32),
          0x00020000);
      const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(x + (ms / 32) * 32 * kSaveRow + (ms % 32) * 8), (short)0, (int)(32 * ldx4 - (ms % 32) * 32),
          0x00020000);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        ma = fmaxf(ma, fabsf(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ares, (int)avo, j * 32, 0))));
      mx = fmaxf(mx, fabsf(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xres, (int)xvo, 0, 0))));
    }
    ma = wave_max_nn(ma);
    mx = wave_max_nn(mx);
    if (lane == 0) {
      wmax[w][0] = ma;
      wmax[w][1] = mx;
    }
    __syncthreads();
    ma = 0.0f;
    mx = 0.0f;
    for (int v = 0; v < kPairWaves; ++v) {
      if ((v >> 3) == half) ma = fmaxf(ma, wmax[v][0]);
      mx = fmaxf(mx, wmax[v][1]);
    }
    Ea = (int)(-block_exp_record(ma)) - kBlockExpBias;
    Ex = (int)(-block_exp_record(mx)) - kBlockExpBias;
  }
  Ea = __builtin_amdgcn_readfirstlane(Ea < kH16EMin ? kH16EMin : Ea);
  Ex = __builtin_amdgcn_readfirstlane(Ex < kH16EMin ? kH16EMin : Ex);
  const float sa = ldexpf(1.0f, 14 - Ea), sx = ldexpf(1.0f, 14 - Ex);

  float ra[2][8], rx[2];
  double bacc = 0.0;                 // bias column (this lane's column, its 8 samples of every stage)
  auto load = [&](auto set_c, int stage) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    const uint32_t rel0 = (uint32_t)(kBfStage * stage) < mrel_end ? (uint32_t)(kBfStage * stage) : mrel_end;
    const int64_t ms = m0 + rel0;
    const bool live = rel0 < mrel_end;   // past the chunk: an empty resource, the loads read zeros
    const __amdgpu_buffer_rsrc_t ares = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a + (ms / 32) * 32 * kGradRow + (ms % 32) * 8), (short)0,
        live ? (int)(32 * lda4 - (ms % 32) * 32) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(x + (ms / 32) * 32 * kSaveRow + (ms % 32) * 8), (short)0,
        live ? (int)(32 * ldx4 - (ms % 32) * 32) : 0, 0x00020000);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      ra[SET][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ares, (int)avo, j * 32, kRowLoadAux));
    rx[SET] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(xres, (int)xvo, 0, kRowLoadAux));
  };
  auto store_x = [&](auto set_c, int buf) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    const float v = rx[SET] * sx;
    const _Float16 hi = (_Float16)v;
    Xs[buf][0][xc][xp] = hi;
    Xs[buf][1][xc][xp] = split_lo(v, hi);
  };
  f32x16 acc[2] = {f32x16{}, f32x16{}};
  const int nstages = (int)((m1 - m0 + 2 * kBfStage - 1) / (2 * kBfStage)) * 2;   // even; the extra reads zeros
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  load(S0{}, 0);
  load(S1{}, 1);
  store_x(S0{}, 0);
  __syncthreads();
  // iteration st: split stage st's a (set st % 2) in registers, reuse the set for stage st+2's loads,
  // stage st's MFMAs (x from LDS buffer st % 2), stage st+1's x into the other buffer
  auto iteration = [&](auto set_c, int st) __attribute__((always_inline)) {
    constexpr int SET = decltype(set_c)::value;
    using Other = std::integral_constant<int, 1 - SET>;
    const int buf = SET;
#pragma unroll
    for (int j = 0; j < 8; ++j) bacc += (double)ra[SET][j];
    h16x8 fh, fl;
    split2_f16(ra[SET], sa, fh, fl);
    load(set_c, st + 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const h16x8 xh = *reinterpret_cast<const h16x8*>(&Xs[buf][0][32 * t + c][8 * h]);
      const h16x8 xl = *reinterpret_cast<const h16x8*>(&Xs[buf][1][32 * t + c][8 * h]);
      f32x16 v = mfma16(fl, xh, acc[t]);   // small products first
      v = mfma16(fh, xl, v);
      acc[t] = mfma16(fh, xh, v);
    }
    store_x(Other{}, buf ^ 1);   // (after the last stage: zeros into the idle buffer)
    __syncthreads();
  };
  for (int st = 0; st < nstages; st += 2) {
    iteration(S0{}, st);
    iteration(S1{}, st + 1);
  }
  // acc = sum (a 2^(14-Ea)) (x 2^(14-Ex)): unscaled here by two exact power-of-two factors (each
  // normal for any exponent the clamps allow)
  const int e = Ea + Ex - 28;
  const float u0 = ldexpf(1.0f, e / 2), u1 = ldexpf(1.0f, e - e / 2);
  constexpr int KP = kPosEnc + 1;
  float* out = partial + (size_t)chunk * wgrad_stride(2 * kHidden, kPosEnc);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int kk = 32 * t + c;
    if (kk < kPosEnc) {
#pragma unroll
      for (int g = 0; g < 16; ++g) out[(size_t)(32 * w + acc_row(g, h)) * KP + kk] = (acc[t][g] * u0) * u1;
    }
  }
  bacc += __shfl_xor(bacc, 32);
  if (h == 0) out[(size_t)(32 * w + c) * KP + kPosEnc] = (float)bacc;
}

// The rgb head's weight gradient (rgb_linear: 3 rows over hd, K = 128) on tile-major rows: a
// streaming kernel, not a GEMM tile (an MFMA tile would keep 3 of its 128 rows).  A workgroup owns a
// chunk of 16 blocks (512 samples); wave w the feature groups 4w..4w+3 of hd.  Per block and group
// a lane reads one float4 (the group's 32 samples x 8 features are 1 KiB contiguous: lane l holds
// sample l/2, features 8g + 4(l&1)..+3) and the sample's d rgb_pre (3 floats), and accumulates the
// 3 x 4 products in double; at the chunk's end the 32 lanes of each parity are summed (shuffles,
// double) into the chunk's partial (N = 3, K = 128 layout of wgrad_reduce_kernel; the bias column
// from wave 0).  Reads hd once at full lines: ~134 MB per 262K-sample step.
// SUMS (rays of N % 32 == 0 samples under the split arithmetic, the fused per-ray sums): the launch
// also writes what the appearance projection's and dir_linear's per-ray GEMMs need from the head,
// since it holds every block's d rgb_pre anyway (models.py:154-160: d hd = W_rgb^T d rgb_pre is linear
// in the sample, so a block's sum of d hd needs only its 3 column sums): per 32-sample block b (all on
// one ray) S_hd[b] = W_rgb^T (the block's d rgb_pre sums, in double, rounded once), and for a ray's
// first block E[ray] = the ray's PE_4(d) (its first sample's save row).  Wave (b - b0) % 4 takes
// block b.  (Until round 6 a separate block_head_sums_kernel read the d rgb_pre rows again.)
template <bool SUMS = false>
__global__ void __launch_bounds__(256)
wgrad_head3_kernel(const float* __restrict__ a, const float* __restrict__ x, int64_t M, float* __restrict__ partial,
                   const float* __restrict__ save = nullptr, const float* __restrict__ packed = nullptr, int N = 0,
                   float* __restrict__ S_hd = nullptr, float* __restrict__ E = nullptr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float wr[3][2];   // SUMS: rgb_linear.weight columns lane, lane + 64
  if constexpr (SUMS) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int q = 0; q < 2; ++q) wr[c][q] = packed[kOffRgbW + c * kDirHidden + 64 * q + lane];
  }
  const int64_t nblk = (M + 31) / 32;
  const int64_t b0 = (int64_t)blockIdx.x * kHeadChunkBlocks;
  const int64_t b1 = b0 + kHeadChunkBlocks < nblk ? b0 + kHeadChunkBlocks : nblk;
  const int j = lane >> 1, par = lane & 1;
  double acc[4][3][4] = {};
  double bacc[3] = {0.0, 0.0, 0.0};
  // the block's rows: gradient rows at d rgb_pre's group, save rows at hd's first group; the next
  // block's loads are issued before this block's products
  auto load = [&](int64_t b, f32x4& dv, f32x4 (&v)[4]) __attribute__((always_inline)) {
    const float* ab = a + b * 32 * kGradRow;
    const float* xb = x + b * 32 * kSaveRow;
    dv = *reinterpret_cast<const f32x4*>(ab + 8 * j);
#pragma unroll
    for (int g = 0; g < 4; ++g) v[g] = *reinterpret_cast<const f32x4*>(xb + (4 * w + g) * 256 + 4 * lane);
  };
  f32x4 dv_n, v_n[4];
  if (b0 < b1) load(b0, dv_n, v_n);
  for (int64_t b = b0; b < b1; ++b) {
    const f32x4 dv = dv_n;
    f32x4 v[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) v[g] = v_n[g];
    if (b + 1 < b1) load(b + 1, dv_n, v_n);
    if constexpr (SUMS) {
      if ((int)((b - b0) & 3) == w) {   // (wave-uniform)
        double ds[3];   // lane (j, par) holds sample j's d rgb_pre: xor 2 .. 32 sums one parity's 32 lanes
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          ds[c] = (double)dv[c];
#pragma unroll
          for (int m = 2; m < 64; m <<= 1) ds[c] += __shfl_xor(ds[c], m);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
          S_hd[b * kDirHidden + 64 * q + lane] =
              (float)(ds[0] * (double)wr[0][q] + ds[1] * (double)wr[1][q] + ds[2] * (double)wr[2][q]);
        if ((b * 32) % N == 0 && lane < 32) E[(b * 32 / N) * 32 + lane] = save[tile_off(b * 32, kSaveEncD + lane, kSaveRow)];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double d = (double)dv[c];
      bacc[c] += par == 0 ? d : 0.0;
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[g][c][e] = fma(d, (double)v[g][e], acc[g][c][e]);
    }
  }
  // sum the 32 lanes of each parity (xor 2 .. 32 keeps the parity), in a fixed order
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int m = 2; m < 64; m <<= 1) acc[g][c][e] += __shfl_xor(acc[g][c][e], m);
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int m = 2; m < 64; m <<= 1) bacc[c] += __shfl_xor(bacc[c], m);
  constexpr int KP = kDirHidden + 1;
  float* out = partial + (size_t)blockIdx.x * wgrad_stride(3, kDirHidden);
  if (lane < 2) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) out[c * KP + 8 * (4 * w + g) + 4 * lane + e] = (float)acc[g][c][e];
    if (w == 0 && lane == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c * KP + kDirHidden] = (float)bacc[c];
    }
  }
}

// The plan's xd1: one x row per sample in a's layout; under BLK a row-major x with x_div == 1 (the
// appearance rows of one-sample "rays") takes the generic x loader, which reads row-major rows.
template <int WN, int WK, bool BLK>
static int launch_wgrad_bf(const WgradGemm& j, const WgradPlan& p, float* ws, hipStream_t s) {
  const int ntn = (j.N + 64 * WN - 1) / (64 * WN), ntk = (j.K + 64 * WK - 1) / (64 * WK);
  const int tiles = ntn * ntk;
  const int blocks = ((p.chunks + 7) / 8) * 8 * tiles;
  if (p.xd1)
    hipLaunchKernelGGL((wgrad_bf_kernel<WN, WK, true, BLK>), dim3((unsigned)blocks), dim3(256), 0, s, j.a, j.lda, j.N, j.x,
                       j.ldx, j.K, j.x_div, j.M, ntk, tiles, p.chunks, p.clen, ws);
  else
    hipLaunchKernelGGL((wgrad_bf_kernel<WN, WK, false, BLK>), dim3((unsigned)blocks), dim3(256), 0, s, j.a, j.lda, j.N, j.x,
                       j.ldx, j.K, j.x_div, j.M, ntk, tiles, p.chunks, p.clen, ws);
  return check_launch("wgrad_bf_kernel");
}

// out_w[n][k] (ld K) and out_b[n] (nullable) = (accumulate ? out : 0) + sum over chunks, in chunk
// order; with a WgradSplit, rows n >= split.n0 go to split.out_w[n - n0][k < split.k] and
// split.out_b[n - n0] instead.  A workgroup owns 64 float4 columns of the partial layout; its
// kRedParts waves each sum a contiguous 1/kRedParts of the chunks (fixed order, eight loads in flight
// per lane), then the parts are added in order: deterministic.  The reductions run beside the other
// stream's GEMMs: eight waves per workgroup made the step 2-3 % slower than four (same-box A/B,
// profiles/r03_ab_train_reduce_parts.log).
constexpr int kRedParts = 4;
__device__ __forceinline__ void wgrad_reduce_body(const float* __restrict__ partial, int chunks, int N, int K,
                                                  float* __restrict__ out_w, int ldo, float* __restrict__ out_b,
                                                  int accumulate, const WgradSplit& split, int scaled) {
  // the chunk partials are added in double and rounded once: a gradient entry is a sum over up to
  // 2^18 samples with heavy cancellation (random-sign upstream gradients), and an fp32 running sum of
  // its 256 chunk partials cost up to ~10x the fp32 CPU autograd's error on the bias columns
  // (tests/test_gpu_accuracy.py::test_gradients_vs_float64, scripts/diag_grad_masks.py)
  typedef double f64x4 __attribute__((ext_vector_type(4)));
  __shared__ f64x4 part[kRedParts][64];
  const int KP = K + 1;
  const int64_t stride = wgrad_stride(N, K);
  const int64_t col4 = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int q = threadIdx.x >> 6;
  const int per = (chunks + kRedParts - 1) / kRedParts;
  const int c0 = q * per < chunks ? q * per : chunks, c1 = c0 + per < chunks ? c0 + per : chunks;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  auto add = [&](const f32x4& v) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += (double)v[e];
  };
  if (col4 * 4 < stride && !scaled) {
    const f32x4* p = reinterpret_cast<const f32x4*>(partial) + col4;
    const int64_t s4 = stride / 4;
    int c = c0;
    for (; c + 8 <= c1; c += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(c + u) * s4];
#pragma unroll
      for (int u = 0; u < 8; ++u) add(v[u]);
    }
    for (; c < c1; ++c) add(p[c * s4]);
  } else if (col4 * 4 < stride) {
    // split-f16 partials: chunk c's values times 2^(its exponent), the bias column as stored (exact in
    // double: powers of two)
    const f32x4* p = reinterpret_cast<const f32x4*>(partial) + col4;
    const int* ex = reinterpret_cast<const int*>(partial) + stride - 4;
    const int64_t s4 = stride / 4;
    bool bias[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bias[e] = (col4 * 4 + e) % (K + 1) == K;
    auto add_scaled = [&](const f32x4& v, int x) __attribute__((always_inline)) {
      const double sc = ldexp(1.0, x);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += bias[e] ? (double)v[e] : (double)v[e] * sc;
    };
    int c = c0;
    for (; c + 8 <= c1; c += 8) {
      f32x4 v[8];
      int x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u] = p[(c + u) * s4];
        x[u] = ex[(c + u) * stride];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) add_scaled(v[u], x[u]);
    }
    for (; c < c1; ++c) add_scaled(p[c * s4], ex[c * stride]);
  }
  part[q][threadIdx.x & 63] = acc;
  __syncthreads();
  if (q != 0 || col4 * 4 >= stride) return;
  f64x4 sum64 = part[0][threadIdx.x];
#pragma unroll
  for (int r = 1; r < kRedParts; ++r) sum64 += part[r][threadIdx.x];
  f32x4 sum;
#pragma unroll
  for (int e = 0; e < 4; ++e) sum[e] = (float)sum64[e];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t idx = col4 * 4 + e;
    if (idx >= (int64_t)N * KP) break;
    const int n = (int)(idx / KP), k = (int)(idx % KP);
    float* dst;
    if (split.out_w && n >= split.n0) {   // rows from n0 on belong to a second output (WgradSplit)
      if (n >= split.n_end) continue;
      const int n2 = n - split.n0;
      dst = k < split.k ? split.out_w + (size_t)n2 * split.ldo + k : (k == K && split.out_b ? split.out_b + n2 : nullptr);
    } else {
      dst = k < K ? out_w + (size_t)n * ldo + k : (out_b ? out_b + n : nullptr);
    }
    if (dst) *dst = accumulate ? *dst + sum[e] : sum[e];
  }
}
__global__ void __launch_bounds__(64 * kRedParts)
wgrad_reduce_kernel(const float* __restrict__ partial, int chunks, int N, int K, float* __restrict__ out_w, int ldo,
                    float* __restrict__ out_b, int accumulate, WgradSplit split, int scaled) {
  wgrad_reduce_body(partial, chunks, N, K, out_w, ldo, out_b, accumulate, split, scaled);
}

template <int WN, int WK, bool BLK>
static int launch_wgrad_lds(const WgradGemm& j, const WgradPlan& p, float* ws, hipStream_t s) {
  const int ntn = (j.N + 64 * WN - 1) / (64 * WN), ntk = (j.K + 64 * WK - 1) / (64 * WK);
  const int tiles = ntn * ntk;
  const int blocks = ((p.chunks + 7) / 8) * 8 * tiles;
  hipLaunchKernelGGL((wgrad_lds_kernel<WN, WK, BLK>), dim3((unsigned)blocks), dim3(256), 0, s, j.a, j.lda, j.N, j.x,
                     j.ldx, j.K, j.x_div, (int)p.x_blk, j.M, ntk, tiles, p.chunks, ws);
  return check_launch("wgrad_lds_kernel");
}

int launch_wgrad_head3(const float* a, const float* x, int64_t M, float* out_w, float* out_b, float* ws,
                       size_t ws_floats, hipStream_t s, const HeadSums* sums) {
  if (M == 0) return NERF_OK;
  const int chunks = wgrad_head3_chunks(M);
  if ((size_t)chunks * wgrad_stride(3, kDirHidden) > ws_floats) return set_error(NERF_ERR_WORKSPACE, "wgrad_head3: workspace");
  if (sums)
    hipLaunchKernelGGL(wgrad_head3_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, s, a, x, M, ws, sums->save,
                       sums->packed, sums->N, sums->S_hd, sums->E);
  else
    hipLaunchKernelGGL(wgrad_head3_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, s, a, x, M, ws);
  if (int rc = check_launch("wgrad_head3_kernel")) return rc;
  const int64_t cols4 = wgrad_stride(3, kDirHidden) / 4;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((cols4 + 63) / 64)), dim3(64 * kRedParts), 0, s, ws, chunks, 3,
                     kDirHidden, out_w, kDirHidden, out_b, 0, WgradSplit{}, 0);
  return check_launch("wgrad_reduce_kernel");
}

// Layer 0's weight gradient (d pre_0 over enc_x) and the skip layer's PE columns (d pre_4 over
// enc_x) as one 512 x 63 split-f16 GEMM over the tile-major rows (wgrad_pair16_kernel): enc_x is read
// once; rows 0..255 go to layer 0's weight + bias, rows 256.. to the skip weight's PE columns.
int launch_wgrad_pe_pair(const float* save, const float* grad, int64_t M, float* w0, float* b0, float* w4, float* ws,
                         size_t ws_floats, hipStream_t s) {
  if (M == 0) return NERF_OK;
  const int clen = wgrad_pair_clen(M), chunks = wgrad_pair_chunks(M);
  if ((size_t)chunks * wgrad_stride(2 * kHidden, kPosEnc) > ws_floats)
    return set_error(NERF_ERR_WORKSPACE, "wgrad pe pair: workspace");
  hipLaunchKernelGGL(wgrad_pair16_kernel, dim3((unsigned)chunks), dim3(64 * kPairWaves), 0, s, grad, save, M, clen, ws);
  if (int rc = check_launch("wgrad_pair16_kernel")) return rc;
  const WgradSplit skip{kHidden, w4 + kHidden, kHidden + kPosEnc, kPosEnc, nullptr};
  const int64_t cols4 = wgrad_stride(2 * kHidden, kPosEnc) / 4;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((cols4 + 63) / 64)), dim3(64 * kRedParts), 0, s, ws, chunks,
                     2 * kHidden, kPosEnc, w0, kPosEnc, b0, 0, skip, 0);
  return check_launch("wgrad_reduce_kernel");
}

// One weight-gradient GEMM (WgradGemm, train_internal.h): the route, the chunks and the reduction's
// mode are wgrad_plan's (wgrad_plan.h), from the shape and the arithmetic in force; here the one launch
// the plan names, then the chunk reduction.
int launch_wgrad(const WgradGemm& j, float* ws, size_t ws_floats, hipStream_t s) {
  if (j.M == 0) return NERF_OK;
  const float *a = j.a, *x = j.x;
  const int64_t lda = j.lda, ldx = j.ldx, x_div = j.x_div, M = j.M;
  const int N = j.N, K = j.K;
  const bool aligned = ((uintptr_t)a % 16 == 0) && ((uintptr_t)x % 16 == 0) && lda % 4 == 0 && ldx % 4 == 0;
  if (j.tiled && !(aligned && lda % 8 == 0 && (x_div != 1 || ldx % 8 == 0)))
    return set_error(NERF_ERR_BAD_ARG, "wgrad: tile-major operands must be aligned with row lengths % 8 == 0");
  const WgradPlan p = wgrad_plan(g_mlp_arith, N, K, x_div, M, lda, ldx, aligned, j.tiled, j.x_tiled);
  if (p.partial_floats > ws_floats) return set_error(NERF_ERR_WORKSPACE, "wgrad: workspace");
  const int chunks = p.chunks, clen = p.clen;
  int rc;
  switch (p.route) {
    case WgradRoute::H16Half:
      if (j.sums)   // (the dir/density launch also writes d pre_dir's 8-sample sums)
        hipLaunchKernelGGL(wgrad_h16h_kernel<true>, dim3((unsigned)((chunks + 7) / 8 * 16)), dim3(256), 0, s, a, lda, x,
                           ldx, M, clen, chunks, N, j.meta, ws, j.sums);
      else
        hipLaunchKernelGGL(wgrad_h16h_kernel<false>, dim3((unsigned)((chunks + 7) / 8 * 16)), dim3(256), 0, s, a, lda, x,
                           ldx, M, clen, chunks, N, j.meta, ws, nullptr);
      rc = check_launch("wgrad_h16h_kernel");
      break;
    case WgradRoute::H16Whole:
      hipLaunchKernelGGL(wgrad_h16w_kernel, dim3((unsigned)chunks), dim3(256), 0, s, a, lda, x, ldx, M, clen, j.meta, ws);
      rc = check_launch("wgrad_h16w_kernel");
      break;
    case WgradRoute::BfK64:
      if (j.tiled)
        hipLaunchKernelGGL(wgrad_bf_k64_kernel<true>, dim3((unsigned)chunks), dim3(512), 0, s, a, lda, x, ldx, K, M,
                           clen, ws);
      else
        hipLaunchKernelGGL(wgrad_bf_k64_kernel<false>, dim3((unsigned)chunks), dim3(512), 0, s, a, lda, x, ldx, K, M,
                           clen, ws);
      rc = check_launch("wgrad_bf_k64_kernel");
      break;
    case WgradRoute::Bf256x64:
      rc = j.tiled ? launch_wgrad_bf<4, 1, true>(j, p, ws, s) : launch_wgrad_bf<4, 1, false>(j, p, ws, s);
      break;
    case WgradRoute::Bf128x128:
      rc = j.tiled ? launch_wgrad_bf<2, 2, true>(j, p, ws, s) : launch_wgrad_bf<2, 2, false>(j, p, ws, s);
      break;
    case WgradRoute::Lds256x64:
      rc = j.tiled ? launch_wgrad_lds<4, 1, true>(j, p, ws, s) : launch_wgrad_lds<4, 1, false>(j, p, ws, s);
      break;
    case WgradRoute::Lds128x128:
      rc = j.tiled ? launch_wgrad_lds<2, 2, true>(j, p, ws, s) : launch_wgrad_lds<2, 2, false>(j, p, ws, s);
      break;
    default: {   // WgradRoute::Fallback
      const int tiles = ((N + 31) / 32) * ((K + 1 + 63) / 64);
      hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)((tiles + 3) / 4), (unsigned)chunks), dim3(256), 0, s, a, lda, N,
                         x, ldx, K, x_div, M, ws);
      rc = check_launch("wgrad_kernel");
    }
  }
  if (rc) return rc;
  if (j.sums && !p.writes_sums) return set_error(NERF_ERR_BAD_ARG, "wgrad: 8-sample sums need the split-f16 whole-tile launch");
  const int64_t cols4 = wgrad_stride(N, K) / 4;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((cols4 + 63) / 64)), dim3(64 * kRedParts), 0, s, ws, chunks, N, K,
                     j.out_w, j.ldo, j.out_b, j.accumulate, j.split, (int)p.scaled);
  return check_launch("wgrad_reduce_kernel");
}

// ------------------------------------------------------------------- appearance gradient
// d app_row(r) = appearance_projection.weight^T . S_r, S_r = sum over the samples that used row r of
// d hd (models.py:154-156: hd += W_app app + b_app).  Row r's samples are src rows
// [r*group, (r+1)*group) with stride ld: per-ray rows pass the gradient rows (group = N); a single
// broadcast row passes the already-reduced bias gradient of appearance_projection (group = 1).
__global__ void __launch_bounds__(128)
app_grad_kernel(const float* __restrict__ src, int64_t ld, int group, int tiled, const float* __restrict__ packed,
                float* __restrict__ dapp) {
  __shared__ float sum[kDirHidden];
  const int64_t r = blockIdx.x;
  const int n = threadIdx.x;
  double acc = 0.0;
  for (int s = 0; s < group; ++s) {
    const int64_t m = r * group + s;     // tiled: gradient rows (layout.h), src at the slice's tile_col
    acc += (double)src[tiled ? tile_off(m, n, (int)ld) : m * ld + n];
  }
  sum[n] = (float)acc;
  __syncthreads();
  if (n < kAppDim) {
    const float* W = packed + kOffAppW;      // (128 x 32) row-major
    float v = 0.0f;
    for (int j = 0; j < kDirHidden; ++j) v = fmaf(W[j * kAppDim + n], sum[j], v);
    dapp[r * kAppDim + n] = v;
  }
}

int launch_app_grad(const float* src, int64_t ld, int64_t rows, int group, const float* packed, float* dapp,
                    hipStream_t s, bool tiled) {
  if (rows == 0) return NERF_OK;
  hipLaunchKernelGGL(app_grad_kernel, dim3((unsigned)rows), dim3(128), 0, s, src, ld, group, (int)tiled, packed, dapp);
  return check_launch("app_grad_kernel");
}

// ---------------------------------------------------------------- per-ray gradient sums
// Inputs that are constant along a ray (PE_4(d) of dir_linear's last 27 columns, the appearance
// row) make their weight gradient a GEMM over rays: sum_m g[m][n] x[ray(m)][k] = sum_r S[r][n] x[r][k]
// with S[r] = sum over the ray's samples of g (distributivity; the sums in double).  Ray r's block:
// S[r] = [sum d pre_dir (128) | sum d hd (128)] from the tile-major gradient rows, and E[r] = the
// ray's PE_4(d) (its first sample's save row, kSaveEncD: 27 values + zeros) as a row-major row.
__global__ void __launch_bounds__(256)
ray_sums_kernel(const float* __restrict__ grad, const float* __restrict__ save, int N, float* __restrict__ S,
                float* __restrict__ E) {
  const int64_t r = blockIdx.x;
  const int t = threadIdx.x;
  const int col = t < kDirHidden ? kGradDir + t : kGradHd + (t - kDirHidden);
  const int64_t m0 = r * N;
  double acc = 0.0;
#pragma unroll 8
  for (int j = 0; j < N; ++j) acc += (double)grad[tile_off(m0 + j, col, kGradRow)];
  S[r * 256 + t] = (float)acc;
  if (t < 32) E[r * 32 + t] = save[tile_off(m0, kSaveEncD + t, kSaveRow)];
}

int launch_ray_sums(const float* grad, const float* save, int64_t B, int N, float* S, float* E, hipStream_t s) {
  hipLaunchKernelGGL(ray_sums_kernel, dim3((unsigned)B), dim3(256), 0, s, grad, save, N, S, E);
  return check_launch("ray_sums_kernel");
}

}  // namespace nerf
