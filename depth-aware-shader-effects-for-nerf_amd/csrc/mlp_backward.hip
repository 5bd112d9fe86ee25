// Training path: the data-gradient chain of NeRF.forward (src/models.py:119-160 differentiated, the
// MLP part of loss.backward(), src/train.py:90), one wave per 32 samples, mirroring the forward
// kernels with transposed weights, and the packers of those weights (nerf_pack_weights_transposed
// and its host twin; layout.h "transposed weights").  Each data-gradient kernel writes every layer's
// d loss / d pre-activation to the tile-major gradient rows (layout.h kGrad*) for the weight gradients (wgrad.hip).
//
//   packT_kernel                  the f32 fragments of W_l^T
//   statsT16_kernel               the split scales and the data-gradient bound constants
//   packT16_kernel                the split-f16 stream; packT_host: the same buffer, bit-identical
//   mlp_backward_kernel           fp32 MFMA, mirroring mlp_kernel (nerf_arith F32)
//   mlp_backward16_kernel         split f16, ReLU masks folded from the saved activations
//                                 (nerf_mlp_backward with masks = NULL)
//   mlp_backward16_bound_kernel   split f16 on the LDS-DMA weight stream of stream16.h with mask
//                                 rows and bound-derived scales: the training step's kernel
//
// The packers share this translation unit with their consumers on purpose.  Alone in a file,
// packT16_word is the only caller of t16_offset (layout.h), the optimizer propagates its argument's
// range into the function before inlining it, and packT16_kernel comes out with other address
// arithmetic (149 instructions either way, different mnemonics); next to mlp_backward16_kernel's
// calls the range stays unknown and the kernel is instruction for instruction what it was.
#include <cstring>

#include "train_internal.h"
#include "stream16.h"

namespace nerf {

// ------------------------------------------------------------------------ transposed weights
NERF_HD inline float packT_value(const float* const* P, size_t e) {
  int mt = (int)(e / (8 * kActSteps * 64));
  if (mt > 7) mt = 7;
  const size_t rel = e - tmat_offset(mt);
  const int j = (int)(rel & 3);
  const int lane = (int)((rel >> 2) & 63);
  const size_t blk = rel >> 8;
  const int ksq = tmat_ksteps(mt) / 4;
  const int nt = (int)(blk / ksq), kq = (int)(blk % ksq);
  const int o = act_feature(4 * kq + j, lane >> 5);       // forward output neuron
  const int i = nt * 32 + (lane & 31);                   // forward input neuron
  if (mt == 7) return P[P_DIR_W][(size_t)o * (kHidden + kDirEnc) + i];
  const int layer = mt + 1;
  const int K = layer == kSkipLayer ? kHidden + kPosEnc : kHidden;
  return P[2 * layer][(size_t)o * K + i];
}

// W^T[i][o] of matrix mt (forward input neuron i, output neuron o)
NERF_HD inline float tmat_weight(const float* const* P, int mt, int i, int o) {
  if (mt == 7) return P[P_DIR_W][(size_t)o * (kHidden + kDirEnc) + i];
  const int layer = mt + 1;
  const int K = layer == kSkipLayer ? kHidden + kPosEnc : kHidden;
  return P[2 * layer][(size_t)o * K + i];
}

// max |W^T| of matrix mt over rows i (one thread per row)
NERF_HD inline float tmat_row_max(const float* const* P, int mt, int i) {
  const int outs = mt == 7 ? kDirHidden : kHidden;
  float m = 0.0f;
  for (int o = 0; o < outs; ++o) m = fmaxf(m, fabsf(tmat_weight(P, mt, i, o)));
  return m;
}

// word w (two halves) of the split-f16 part, w relative to t16_offset(0)
NERF_HD inline uint32_t packT16_word(const float* const* P, const float* consts, size_t w) {
  const size_t c = w / kChunkFloats;                    // chunk of the stream
  const int mt = c < 8 ? 7 : 6 - (int)((c - 8) / 16);
  const size_t rel = w - (t16_offset(mt) - kPackedT32Floats);
  const int KS = t16_ksteps(mt);
  const int jj = (int)(rel & 3), lane = (int)((rel >> 2) & 63);
  const size_t piece = rel >> 8;
  const int part = (int)(piece & 1), i = (int)((piece >> 1) & 3);
  const int step = (int)(piece >> 3), g = step / KS, ks = step % KS;
  const int row = 32 * (4 * g + i) + (lane & 31);
  uint32_t word = 0;
  for (int k = 0; k < 2; ++k) {
    const int j = 2 * jj + k;
    const int o = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3);
    const float v = tmat_weight(P, mt, row, o) * consts[mt];
    const _Float16 hi = (_Float16)v;
    const _Float16 out = part == 0 ? hi : (_Float16)(v - (float)hi);
    uint16_t bits;
    memcpy(&bits, &out, 2);
    word |= (uint32_t)bits << (16 * k);
  }
  return word;
}

struct ParamPtrsT { const float* p[P_COUNT]; };

// (the last block also zeroes the split stream's constant slots, which statsT16_kernel's atomics fill)
__global__ void __launch_bounds__(256) packT_kernel(ParamPtrsT P, float* __restrict__ packed) {
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x < kT16Consts) packed[kOffT16Consts + threadIdx.x] = 0.0f;
    return;
  }
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < kPackedT32Floats) packed[e] = packT_value(P.p, e);
}

// Statistics of the split scales (statsT16_kernel below): max |W^T| of matrix mt (= max |W| over its
// columns i < kHidden), 8 rows of W^T per block (thread = row i, coalesced over i), combined by
// atomicMax on the float bits (exact in any order) into consts[mt] (zeroed first); the last block
// turns the maxima into s_w and 1/s_w.
// Row L1 norm of W^T (a forward input neuron's weights over the outputs): four partial sums over
// the output quarters, each in order, added in order (the host's tmat_row_l1 is the same
// expression, so device and host constants are bit-identical); the matrix's maximum by atomicMax on
// the float bits (exact in any order).  One block per (matrix, 64 rows): thread = (row, quarter).
// One more block takes max |density_head.weight|.
NERF_HD inline float tmat_row_l1_part(const float* const* P, int mt, int i, int q) {
  const int outs = mt == 7 ? kDirHidden : kHidden, per = outs / 4;
  float l1 = 0.0f;
  for (int o = q * per; o < (q + 1) * per; ++o) l1 += fabsf(tmat_weight(P, mt, i, o));
  return l1;
}
NERF_HD inline float tmat_row_l1(const float* const* P, int mt, int i) {
  return ((tmat_row_l1_part(P, mt, i, 0) + tmat_row_l1_part(P, mt, i, 1)) + tmat_row_l1_part(P, mt, i, 2)) +
         tmat_row_l1_part(P, mt, i, 3);
}

// The three statistics passes in one launch (formerly scaleT16 / boundT16 / finalize kernels): the
// block counter (an unused constant slot, zeroed by packT_kernel, reset after) elects the last block
// to finish, which turns the maxima into the constants.  Blocks 0..255: max |W^T| (matrix b / 32,
// outputs 8 (b % 32) ..); 256..287: row L1 norms (matrix (b - 256) / 4); 288: max |density weight|.
constexpr int kT16Counter = kT16Consts - 1;
static_assert(kT16Counter > kT16WsigMax, "the counter slot is unused by the constants");
__global__ void __launch_bounds__(256) statsT16_kernel(ParamPtrsT P, float* __restrict__ packed) {
  __shared__ float part[4][64];
  __shared__ unsigned last;
  unsigned* c = reinterpret_cast<unsigned*>(packed + kOffT16Consts);
  const int b = blockIdx.x;
  if (b < 256) {
    const int mt = b / 32, i = threadIdx.x;
    const int outs = mt == 7 ? kDirHidden : kHidden;
    const int o0 = (b % 32) * 8;
    float m = 0.0f;
    for (int o = o0; o < o0 + 8 && o < outs; ++o) m = fmaxf(m, fabsf(tmat_weight(P.p, mt, i, o)));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) {
      atomicMax(c + mt, __float_as_uint(m));
      __threadfence();
    }
  } else if (b == 256 + 32) {
    float v = fabsf(P.p[P_SIGMA_W][threadIdx.x]);
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) {
      atomicMax(c + kT16WsigMax, __float_as_uint(v));
      __threadfence();
    }
  } else {
    const int bb = b - 256, mt = bb >> 2, r = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = (bb & 3) * 64 + r;
    part[q][r] = tmat_row_l1_part(P.p, mt, i, q);
    __syncthreads();
    if (q == 0) {
      float v = ((part[0][r] + part[1][r]) + part[2][r]) + part[3][r];
      for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
      if (r == 0) {
        atomicMax(c + kT16C + mt, __float_as_uint(v));
        __threadfence();
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(c + kT16Counter, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!last) return;   // (uniform)
  __threadfence();
  if (threadIdx.x < 8) {
    const int mt = threadIdx.x;
    const float mx = __uint_as_float(__hip_atomic_load(c + mt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const float l1 = __uint_as_float(__hip_atomic_load(c + kT16C + mt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    store_t16_consts(packed + kOffT16Consts, mt, mx);
    packed[kOffT16Consts + kT16C + mt] = l1 * 1.0001f;   // rounding margin on the float sums: a bound
  }
  if (threadIdx.x == 0) __hip_atomic_store(c + kT16Counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) packT16_kernel(ParamPtrsT P, float* __restrict__ packed) {
  const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < kOffT16Consts - kPackedT32Floats)
    reinterpret_cast<uint32_t*>(packed)[kPackedT32Floats + w] = packT16_word(P.p, packed + kOffT16Consts, w);
}

int launch_packT(const float* const* params, float* packedT, hipStream_t s) {
  ParamPtrsT P;
  for (int i = 0; i < P_COUNT; ++i) P.p[i] = params[i];
  hipLaunchKernelGGL(packT_kernel, dim3((unsigned)((kPackedT32Floats + 255) / 256 + 1)), dim3(256), 0, s, P, packedT);
  if (int rc = check_launch("packT_kernel")) return rc;
  hipLaunchKernelGGL(statsT16_kernel, dim3(256 + 33), dim3(256), 0, s, P, packedT);
  if (int rc = check_launch("statsT16_kernel")) return rc;
  const size_t words = kOffT16Consts - kPackedT32Floats;
  hipLaunchKernelGGL(packT16_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, P, packedT);
  return check_launch("packT16_kernel");
}

void packT_host(const float* const* params, float* packedT) {
  for (size_t e = 0; e < kPackedT32Floats; ++e) packedT[e] = packT_value(params, e);
  float* consts = packedT + kOffT16Consts;
  for (int k = 0; k < kT16Consts; ++k) consts[k] = 0.0f;
  for (int mt = 0; mt < 8; ++mt) {
    float mx = 0.0f, l1 = 0.0f;
    for (int i = 0; i < kHidden; ++i) {
      mx = fmaxf(mx, tmat_row_max(params, mt, i));
      l1 = fmaxf(l1, tmat_row_l1(params, mt, i));
    }
    store_t16_consts(consts, mt, mx);
    consts[kT16C + mt] = l1 * 1.0001f;
  }
  for (int i = 0; i < kHidden; ++i) consts[kT16WsigMax] = fmaxf(consts[kT16WsigMax], fabsf(params[P_SIGMA_W][i]));
  uint32_t* words = reinterpret_cast<uint32_t*>(packedT);
  for (size_t w = 0; w < kOffT16Consts - kPackedT32Floats; ++w)
    words[kPackedT32Floats + w] = packT16_word(params, consts, w);
}

// ------------------------------------------------------------------------------ MLP backward
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// out (8 tiles, 256 forward-input neurons) = W^T . in (KS k-steps of forward-output neurons in
// accumulator order), from a transposed fragment matrix.  Four tiles interleaved (independent
// MFMAs); weights streamed through a DEPTH-block register ring.
template <int KS>
__device__ __forceinline__ void dgrad(const float* __restrict__ wmat, const f32x16 (&in)[8], f32x16 (&out)[8],
                                      int lane) {
  constexpr int KSQ = KS / 4;
  constexpr int DEPTH = 8;
  constexpr int G = 8 * KSQ;
  const f32x4* __restrict__ wf = reinterpret_cast<const f32x4*>(wmat) + lane;
  auto blk = [](int g) { return ((g / (4 * KSQ)) * 4 + g % 4) * KSQ + (g / 4) % KSQ; };
  f32x4 ring[DEPTH];
#pragma unroll
  for (int p = 0; p < DEPTH; ++p) ring[p] = wf[blk(p) * 64];
  static_for<G / 4>([&](auto sc) __attribute__((always_inline)) {
    constexpr int st = decltype(sc)::value;
    constexpr int grp = st / KSQ, kq = st % KSQ;
    if constexpr (kq == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) out[4 * grp + i] = f32x16{};
    }
    static_for<4>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      constexpr int ks = 4 * kq + j;
      const float b = in[ks >> 4][ks & 15];
      static_for<4>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        out[4 * grp + i] = mfma32t(ring[(4 * st + i) % DEPTH][j], b, out[4 * grp + i]);
      });
    });
    static_for<4>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      constexpr int g = 4 * st + i;
      if constexpr (g + DEPTH < G) ring[g % DEPTH] = wf[blk(g + DEPTH) * 64];
    });
    __builtin_amdgcn_sched_barrier(0);
  });
}

// A wave's 32 gradient rows as a buffer resource sized to the rows that exist, so the stores of
// tail lanes fall outside it and are dropped: no branches around stores, which would otherwise
// split the loads and stores of the ReLU backward into one memory round trip per 16 bytes.
struct GradRows {
  __amdgpu_buffer_rsrc_t res;
  uint32_t loff;   // this lane's byte offset: row (lane & 31), lane half h
};

// (tile-major rows, layout.h: the wave's block of 32 samples; a lane's 4 features of a group at
// ((lane & 31) 8 + 4h) floats; a lane past M, or a wave past M, stores nothing)
__device__ __forceinline__ GradRows grad_rows(float* grad, int64_t s0, int64_t M, int lane) {
  const bool any = s0 < M;
  GradRows g;
  g.res = __builtin_amdgcn_make_buffer_rsrc(grad + (any ? s0 : 0) * kGradRow, (short)0, any ? 32 * kGradRow * 4 : 0,
                                            0x00020000);
  g.loff = s0 + (lane & 31) < M ? ((uint32_t)(lane & 31) * 8 + 4 * (uint32_t)(lane >> 5)) * 4 : 0x40000000u;
  return g;
}

// Sample s's place in its tile-major block: element f of the row at tile_row(...) + tile_col(f) + f % 8.
template <typename T>
__device__ __forceinline__ T* tile_row(T* base, int64_t s, int R) {
  return base + (s / 32) * 32 * (int64_t)R + (s % 32) * 8;
}

// 16 bytes at feature off (+ 4 h) of this lane's gradient row (off a multiple of 8)
__device__ __forceinline__ void grad_store4(const GradRows& g, int off, f32x4 v) {
  store16_rows<0>(v, g.res, g.loff + 4u * (uint32_t)tile_col(off));
}

// d pre-activation = d activation * [activation > 0] (ReLU backward; the saved activation is
// ReLU(pre), positive exactly where pre is), in place, and stored to the gradient row.
__device__ __forceinline__ void relu_back_store(f32x16 (&x)[8], int ntiles, const float* __restrict__ srow,
                                                int save_off, const GradRows& gr, int grad_off, int h) {
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    if (t >= ntiles) break;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(srow + tile_col(save_off + t * 32 + 8 * q) + 4 * h);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = a[e] > 0.0f ? x[t][4 * q + e] : 0.0f;
        x[t][4 * q + e] = d;
        v[e] = d;
      }
      grad_store4(gr, grad_off + t * 32 + 8 * q, v);
    }
  }
}

__global__ void __launch_bounds__(256, 1)
mlp_backward_kernel(const float* __restrict__ packed, const float* __restrict__ packedT,
                    const float* __restrict__ save, const float* __restrict__ sigma, const float* __restrict__ rgb,
                    const float* __restrict__ dsigma, const float* __restrict__ drgb, int64_t M,
                    float* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * 32;   // wave-uniform
  if (s0 >= M) return;
  const int h = lane >> 5;
  const int64_t s = imin64(s0 + (lane & 31), M - 1);
  const bool valid = s0 + (lane & 31) < M;
  const float* srow = tile_row(save, s, kSaveRow);
  float* grow = tile_row(grad, s, kGradRow);
  const GradRows gr = grad_rows(grad, s0, M, lane);

  // rgb head: rgb = sigmoid(v) -> dv = drgb * rgb (1 - rgb) (models.py:159-160)
  float dv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float y = rgb[3 * s + c];
    dv[c] = drgb[3 * s + c] * (y * (1.0f - y));
  }
  // density head: sigma = ReLU(v_s) -> d v_s = dsigma * [sigma > 0]
  const float dsp = sigma[s] > 0.0f ? dsigma[s] : 0.0f;
  if (valid && h == 0) {
    grow[tile_col(kGradSigma)] = dsp;
    grow[tile_col(kMetaGradF) + kMetaGradF % 8] = 0.0f;   // no block exponent (layout.h)
#pragma unroll
    for (int c = 0; c < 3; ++c) grow[tile_col(kGradRgb) + c] = dv[c];
  }
  f32x16 A[8], B[8];
  // d hd = W_rgb^T dv (128, accumulator layout in A[0..3])
  const float* wr = packed + kOffRgbW;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = t * 32 + 8 * q + 4 * h + e;
        const float d = fmaf(dv[2], wr[2 * kDirHidden + n], fmaf(dv[1], wr[kDirHidden + n], dv[0] * wr[n]));
        A[t][4 * q + e] = d;
        v[e] = d;
      }
      grad_store4(gr, kGradHd + t * 32 + 8 * q, v);
    }
  // hd = ReLU(dir pre) + appearance: d dir_pre = d hd * [r_dir > 0]
  relu_back_store(A, 4, srow, kSaveRDir, gr, kGradDir, h);
  // d h7 = W_dh^T d dir_pre + w_sigma * d v_s
  dgrad<kDirHidden / 2>(packedT + tmat_offset(7), A, B, lane);
  const float* wsg = packed + kOffSigmaW;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(wsg + t * 32 + 8 * q + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) B[t][4 * q + e] = fmaf(dsp, w[e], B[t][4 * q + e]);
    }
  // trunk, top down: d pre_l = d h_l [h_l > 0]; d h_{l-1} = W_l^T d pre_l
#pragma unroll 1
  for (int p = 0; p < 3; ++p) {
    const int l1 = 7 - 2 * p, l2 = 6 - 2 * p;
    relu_back_store(B, 8, srow, save_h(l1), gr, l1 * kHidden, h);
    dgrad<kActSteps>(packedT + tmat_offset(l1 - 1), B, A, lane);
    relu_back_store(A, 8, srow, save_h(l2), gr, l2 * kHidden, h);
    dgrad<kActSteps>(packedT + tmat_offset(l2 - 1), A, B, lane);
  }
  relu_back_store(B, 8, srow, save_h(1), gr, 1 * kHidden, h);
  dgrad<kActSteps>(packedT + tmat_offset(0), B, A, lane);
  relu_back_store(A, 8, srow, save_h(0), gr, 0, h);
}

// ---------------------------------------------------------------- MLP backward, split f16
// The same chain on v_mfma_f32_32x32x16_f16 (nerf_arith F16X3), the arithmetic of mlp16_kernel:
// out = W^T g as hi(W s_w) hi(g s_g) + hi(W s_w) lo(g s_g) + lo(W s_w) hi(g s_g) with f32
// accumulation, unscaled by the exact inverses.  x s = hi + lo + O(2^-24 |x s|) for both operands
// and the dropped lo lo term is O(2^-22) of the products, so the result has fp32-level error.
// s_w is per matrix (pack time, packedT's split part); s_g is per sample, from the exact max |g|
// over the sample's gradient row (both lane halves): the whole row exists before the layer starts,
// so no bound is needed.  s_g = 2^(140 - E), E the biased exponent of the max (>= 14, so s_g stays
// a normal float): |g s_g| < 2^14.  Each 16-deep k-step is 3 x 32 MFMA cycles against 8 x 64 for
// v_mfma_f32_32x32x2_f32.  Weights stream per wave from L2 through a 3-step register ring (one
// step = 4 tiles x {hi, lo} = 8 KiB for 12 MFMAs).

__device__ __forceinline__ f32x16 mfma16t(u32x4 a, h16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, a), b, c, 0, 0, 0);
}

// Split tiles 0..NT-1 of X (k-steps 2t + s: accumulator elements 8s..8s+7) at the sample's scale,
// negative for odd samples (lane & 1; see mlp_backward16_bound_kernel); returns 1 / s_g.
template <int NT>
__device__ __forceinline__ float split_rows(const f32x16 (&X)[8], h16x8 (&bh)[16], h16x8 (&bl)[16]) {
  float m = 0.0f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) m = fmaxf(m, fabsf(X[t][g]));
  m = fmaxf(m, __shfl_xor(m, 32));
  int E = (int)((__float_as_uint(m) >> 23) & 0xffu);
  E = E < 14 ? 14 : E;
  const float sgn = (threadIdx.x & 1) ? -1.0f : 1.0f;
  const float sc = sgn * __uint_as_float((uint32_t)(267 - E) << 23);
  typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int j = 0; j < 8; j += 2) {   // a pair: hi by one v_cvt_pk_f16_f32, lo by split_lo_pair
        const float v0 = X[t][8 * q + j] * sc, v1 = X[t][8 * q + j + 1] * sc;
        const h16x2 hi2 = {(_Float16)v0, (_Float16)v1};
        const h16x2 lo2 = __builtin_bit_cast(h16x2, split_lo_pair(__builtin_bit_cast(uint32_t, hi2), v0, v1));
        bh[2 * t + q][j] = hi2[0];
        bh[2 * t + q][j + 1] = hi2[1];
        bl[2 * t + q][j] = lo2[0];
        bl[2 * t + q][j + 1] = lo2[1];
      }
  return sgn * __uint_as_float((uint32_t)(E - 13) << 23);
}

// out (8 tiles) = (W^T g) from the split operands of KS k-steps; inv_w = 1/s_w, inv_g = 1/s_g.
// Meanwhile the output's ReLU mask is fetched: the 128 saved activations this lane needs next
// (act, 32 chunks of 4 at act + 32 t + 8 q) are loaded a few per step and folded into 128 bits
// (chunk c = 4 t + q, element e -> bit 4 c + e), so the ReLU backward waits for no load.
__device__ __forceinline__ void fold_mask(uint32_t (&mask)[4], int c, f32x4 a) {
#pragma unroll
  for (int e = 0; e < 4; ++e) mask[c / 8] |= (a[e] > 0.0f ? 1u : 0u) << (4 * (c % 8) + e);
}

// (Without mask rows: nerf_mlp_backward called with masks = NULL.  The training path runs
// mlp_backward16_bound_kernel below.)
template <int KS>
__device__ __forceinline__ void dgrad16(const uint32_t* __restrict__ wmat, const h16x8 (&bh)[16],
                                        const h16x8 (&bl)[16], f32x16 (&out)[8], float inv_w, float inv_g,
                                        const float* __restrict__ act, uint32_t (&mask)[4], int lane) {
  constexpr int STEPS = 2 * KS, PIECES = 8 * STEPS, DEPTH = 24;
  constexpr int CPS = 32 / STEPS, LAG = 3, RS = (LAG + 1) * CPS;   // mask chunks per step, load->fold lag
  const u32x4* __restrict__ wf = reinterpret_cast<const u32x4*>(wmat) + lane;
  u32x4 ring[DEPTH];
  f32x4 pf[RS];
#pragma unroll
  for (int i = 0; i < 4; ++i) mask[i] = 0u;
#pragma unroll
  for (int p = 0; p < DEPTH; ++p) ring[p] = wf[p * 64];
  static_for<STEPS>([&](auto sc) __attribute__((always_inline)) {
    constexpr int st = decltype(sc)::value;
    constexpr int g = st / KS, ks = st % KS;
    if constexpr (st >= LAG) {
#pragma unroll
      for (int u = 0; u < CPS; ++u) fold_mask(mask, (st - LAG) * CPS + u, pf[((st - LAG) * CPS + u) % RS]);
    }
#pragma unroll
    for (int u = 0; u < CPS; ++u) {
      const int c = st * CPS + u;
      pf[c % RS] = *reinterpret_cast<const f32x4*>(act + 256 * c);   // tile-major: feature group c
    }
    if constexpr (ks == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) out[4 * g + i] = f32x16{};
    }
    // small products first: lo(W) hi(g), hi(W) lo(g), then hi(W) hi(g); tiles interleaved
    static_for<4>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      out[4 * g + i] = mfma16t(ring[(8 * st + 2 * i + 1) % DEPTH], bh[ks], out[4 * g + i]);
    });
    static_for<4>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      out[4 * g + i] = mfma16t(ring[(8 * st + 2 * i) % DEPTH], bl[ks], out[4 * g + i]);
    });
    static_for<4>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      out[4 * g + i] = mfma16t(ring[(8 * st + 2 * i) % DEPTH], bh[ks], out[4 * g + i]);
    });
    static_for<8>([&](auto qc) __attribute__((always_inline)) {
      constexpr int p = 8 * st + decltype(qc)::value;
      if constexpr (p + DEPTH < PIECES) ring[p % DEPTH] = wf[(p + DEPTH) * 64];
    });
    if constexpr (ks == KS - 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) out[4 * g + i] = (out[4 * g + i] * inv_w) * inv_g;
    }
    __builtin_amdgcn_sched_barrier(0);
  });
#pragma unroll
  for (int c = (STEPS - LAG) * CPS; c < 32; ++c) fold_mask(mask, c, pf[c % RS]);
}

// relu_back_store with the mask from dgrad16 (tiles 0..NT-1)
template <int NT = 8>
__device__ __forceinline__ void relu_mask_store(f32x16 (&x)[8], const uint32_t (&mask)[4], const GradRows& gr,
                                                int grad_off) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 4 * t + q;
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = (mask[c / 8] >> (4 * (c % 8) + e)) & 1u ? x[t][4 * q + e] : 0.0f;
        x[t][4 * q + e] = d;
        v[e] = d;
      }
      grad_store4(gr, grad_off + t * 32 + 8 * q, v);
    }
}

// Data gradient under f16x3 without mask rows (nerf_mlp_backward with masks = NULL): ReLU masks
// folded from the saved f32 activations, W^T fragments loaded per wave.
__global__ void __launch_bounds__(256, 1)
mlp_backward16_kernel(const float* __restrict__ packed, const float* __restrict__ packedT,
                      const float* __restrict__ save, const float* __restrict__ sigma, const float* __restrict__ rgb,
                      const float* __restrict__ dsigma, const float* __restrict__ drgb, int64_t M,
                      float* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * 32;   // wave-uniform
  if (s0 >= M) return;
  const int h = lane >> 5;
  const int64_t s = imin64(s0 + (lane & 31), M - 1);
  const bool valid = s0 + (lane & 31) < M;
  const float* srow = tile_row(save, s, kSaveRow);
  float* grow = tile_row(grad, s, kGradRow);
  const GradRows gr = grad_rows(grad, s0, M, lane);
  const uint32_t* t16 = reinterpret_cast<const uint32_t*>(packedT);
  const float* invw = packedT + kOffT16Consts + 8;

  // heads, as mlp_backward_kernel
  float dv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float y = rgb[3 * s + c];
    dv[c] = drgb[3 * s + c] * (y * (1.0f - y));
  }
  const float dsp = sigma[s] > 0.0f ? dsigma[s] : 0.0f;
  if (valid && h == 0) {
    grow[tile_col(kGradSigma)] = dsp;
    grow[tile_col(kMetaGradF) + kMetaGradF % 8] = 0.0f;   // no block exponent (layout.h)
#pragma unroll
    for (int c = 0; c < 3; ++c) grow[tile_col(kGradRgb) + c] = dv[c];
  }
  f32x16 X[8];
  h16x8 bh[16], bl[16];
  const float* wr = packed + kOffRgbW;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = t * 32 + 8 * q + 4 * h + e;
        const float d = fmaf(dv[2], wr[2 * kDirHidden + n], fmaf(dv[1], wr[kDirHidden + n], dv[0] * wr[n]));
        X[t][4 * q + e] = d;
        v[e] = d;
      }
      grad_store4(gr, kGradHd + t * 32 + 8 * q, v);
    }
  uint32_t mask[4];
  relu_back_store(X, 4, srow, kSaveRDir, gr, kGradDir, h);
  float inv_g = split_rows<4>(X, bh, bl);
  dgrad16<kDirHidden / 16>(t16 + t16_offset(7), bh, bl, X, invw[7], inv_g, srow + tile_col(save_h(7)) + 4 * h, mask, lane);
  const float* wsg = packed + kOffSigmaW;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(wsg + t * 32 + 8 * q + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) X[t][4 * q + e] = fmaf(dsp, w[e], X[t][4 * q + e]);
    }
#pragma unroll 1
  for (int l = 7; l >= 1; --l) {
    relu_mask_store(X, mask, gr, l * kHidden);
    inv_g = split_rows<8>(X, bh, bl);
    dgrad16<kHidden / 16>(t16 + t16_offset(l - 1), bh, bl, X, invw[l - 1], inv_g, srow + tile_col(save_h(l - 1)) + 4 * h, mask,
                          lane);
  }
  relu_mask_store(X, mask, gr, 0);
}

// ---- data gradient with split scales from a bound (f16x3, mask rows: the training path) ---------
// A split scale taken from the exact maximum of the layer's whole gradient row (round 2's kernel,
// in git history) leaves no output convertible before the last MFMA of the layer: the epilogue
// (mask, row store, maximum, split) sits exposed between layers (PMC: MFMA busy 25 %, 47 % of wave
// cycles in dependency waits).  Here the scale of d pre_{l-1} = mask . (W_l^T d pre_l)
// comes from the bound |W_l^T g| <= C_l max|g|, C_l the largest row L1 norm of W_l^T (pack-time,
// packedT kT16C), with max|g| the exact maximum of this layer's input, tracked while that input was
// being converted.  So the schedule is mlp16_kernel's (stream16.h): a layer's 8 output tiles run as
// two groups of 4 over all 16 k-steps; group A's side work converts the previous layer's tiles 4-7
// into operands 8..15, group B's converts this layer's tiles 0-3 into operands 0..7, each a quarter
// tile per half-step in the MFMA shadow.  A quarter: unscale, (layer 7: + dsigma w_sigma), ReLU mask
// from the forward's mask row, one 16-byte store of the gradient row, running max, split.  A loose
// bound only lowers the split's absolute error floor (2^-25 of the scaled unit: for a bound 2^k
// above the row's maximum, 2^(k-39) of that maximum), far below fp32 rounding.
// The head (rgb sigmoid, density ReLU, W_rgb^T, r_dir mask) and the dir layer's input split run
// first on the VALU; the dir layer's inputs sit in operands 8..15 (the dir layer has 8 k-steps), so
// its group B converts dh_7 tiles 0-3 straight into operands 0..7 for layer 7.
constexpr int kBoLdsMask = 4 * kChunkFloats;                          // after the 4-slot ring
constexpr int kBoLdsWsig = kBoLdsMask + 4 * 32 * kMaskRow;            // density-head weights (256)
constexpr int kBoLdsConsts = kBoLdsWsig + kHidden;                    // packedT's 32 constants
constexpr int kBoLdsFloats = kBoLdsConsts + kT16Consts;               // 99.6 KiB

struct GradAt {                      // where a layer's d pre-activations go, and its mask
  __amdgpu_buffer_rsrc_t rows;       // the wave's gradient rows (tail rows outside: stores dropped)
  uint32_t loff;                     // this lane's byte offset in the tile-major block: ((lane & 31) 8 + 4h) 4
  int slice;                         // the layer's first float in the row, uniform
  const uint32_t* mrow;              // this lane's mask words in LDS (sample row + 4h words)
  int mlay;                          // the layer's words in the row: 8 * layer, uniform
};
struct BwQuarter {
  uint32_t mw;                       // the quarter's mask word
  f32x4 w;                           // (layer 7) density-head weights
};

template <int T0, int QG, bool SIGMA>
__device__ __forceinline__ void bw_load4(const GradAt& g, const float* wsig, int h, BwQuarter& qv) {
  constexpr int T = T0 + QG / 4, q = QG % 4;
  qv.mw = g.mrow[g.mlay + T / 2];
  if constexpr (SIGMA) qv.w = *reinterpret_cast<const f32x4*>(wsig + 32 * T + 8 * q + 4 * h);
}

// Quarter QG of a 4-tile group = registers 4q..4q+3 of output tile T0 + QG/4 -> elements 4(q&1)..+3
// of operand in[OP0 + QG/2] (the forward's convert4 with the backward's epilogue).
template <int T0, int OP0, int QG, bool SIGMA, bool SPLIT>
__device__ __forceinline__ void bw_convert4(const f32x16 (&acc)[8], float inv, float dsp, const BwQuarter& qv,
                                            float s, Operand (&in)[16], float& m, const GradAt& g) {
  constexpr int T = T0 + QG / 4, q = QG % 4;
  constexpr int SH = 16 * (T % 2) + 4 * q;
  f32x4 dv;
  float xs[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float x = acc[T][4 * q + e] * inv;
    if constexpr (SIGMA) x = fmaf(dsp, qv.w[e], x);
    const float d = (qv.mw >> (SH + e)) & 1u ? x : 0.0f;
    dv[e] = d;
    m = fmaxf(m, fabsf(d));          // (layer 0, SPLIT = false: its block exponent record)
    if constexpr (SPLIT) xs[e] = d * s;
  }
  store16_rows<kRowStoreAux, true>(dv, g.rows,
                                   g.loff + 4u * (uint32_t)tile_col(g.slice) + 4u * (uint32_t)tile_col(32 * T + 8 * q));
  if constexpr (SPLIT) {   // hi pairs by v_cvt_pk_f16_f32, lo pairs by split_lo_pair
    Operand& op = in[OP0 + QG / 2];
    typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const h16x2 hi2 = {(_Float16)xs[2 * p], (_Float16)xs[2 * p + 1]};
      const h16x2 lo2 =
          __builtin_bit_cast(h16x2, split_lo_pair(__builtin_bit_cast(uint32_t, hi2), xs[2 * p], xs[2 * p + 1]));
      const int j = 4 * (q & 1) + 2 * p;
      op.hi[j] = hi2[0];
      op.hi[j + 1] = hi2[1];
      op.lo[j] = lo2[0];
      op.lo[j + 1] = lo2[1];
    }
  }
}

template <int PH, int T0, int OP0, int QG, bool SIGMA, bool SPLIT>
__device__ __forceinline__ void bw_quarter(const f32x16 (&acc)[8], float inv, float dsp, const float* wsig, int h,
                                           float s, Operand (&in)[16], float& m, BwQuarter& qv, const GradAt& g) {
  if constexpr (PH == 0) bw_load4<T0, QG, SIGMA>(g, wsig, h, qv);
  else bw_convert4<T0, OP0, QG, SIGMA, SPLIT>(acc, inv, dsp, qv, s, in, m, g);
}

__global__ void __launch_bounds__(64 * kW16Waves, 1)
mlp_backward16_bound_kernel(const float* __restrict__ packed, const float* __restrict__ packedT,
                            const uint32_t* __restrict__ masks, const float* __restrict__ sigma,
                            const float* __restrict__ rgb, const float* __restrict__ dsigma,
                            const float* __restrict__ drgb, int64_t M, float* __restrict__ grad, int store_dhd) {
  __shared__ __attribute__((aligned(16))) float lds[kBoLdsFloats];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, h = lane >> 5;
  const int64_t s0 = ((int64_t)blockIdx.x * kW16Waves + wave) * 32;
  // every wave runs to the end (the weight stream has barriers); tail lanes repeat sample M-1 and
  // store nothing
  const bool valid = s0 + (lane & 31) < M;
  const int64_t s = imin64(s0 + (lane & 31), M - 1);
  GradAt ga;                          // the wave's tile-major block (layout.h)
  ga.rows = __builtin_amdgcn_make_buffer_rsrc(grad + (s0 < M ? s0 : 0) * kGradRow, (short)0,
                                              s0 < M ? 32 * kGradRow * 4 : 0, 0x00020000);
  ga.loff = valid ? ((uint32_t)(lane & 31) * 8 + 4 * h) * 4 : 0x40000000u;
  // the wave's 32 mask rows (8,704 contiguous bytes) into LDS; constants and w_sigma
  uint32_t* mwave = reinterpret_cast<uint32_t*>(lds + kBoLdsMask) + wave * 32 * kMaskRow;
  for (int i = lane; i < 32 * kMaskRow / 4; i += 64) {
    const int row = i / (kMaskRow / 4), c = i % (kMaskRow / 4);
    reinterpret_cast<u32x4*>(mwave)[i] = reinterpret_cast<const u32x4*>(masks + imin64(s0 + row, M - 1) * kMaskRow)[c];
  }
  if (threadIdx.x < kHidden / 4)
    reinterpret_cast<f32x4*>(lds + kBoLdsWsig)[threadIdx.x] = reinterpret_cast<const f32x4*>(packed + kOffSigmaW)[threadIdx.x];
  if (threadIdx.x < kT16Consts) lds[kBoLdsConsts + threadIdx.x] = packedT[kOffT16Consts + threadIdx.x];
  ga.mrow = mwave + (lane & 31) * kMaskRow + 4 * h;
  ga.mlay = 0;
  ga.slice = 0;

  // heads (models.py:137-160 differentiated): rgb = sigmoid(v) -> dv = drgb rgb (1 - rgb); density
  // sigma = ReLU(v_s) -> d v_s = dsigma [sigma > 0]
  float dv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float y = rgb[3 * s + c];
    dv[c] = drgb[3 * s + c] * (y * (1.0f - y));
  }
  const float dsp = sigma[s] > 0.0f ? dsigma[s] : 0.0f;
  const float* wr = packed + kOffRgbW;
  float dhd[4][16];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = t * 32 + 8 * q + 4 * h + e;
        dhd[t][4 * q + e] = fmaf(dv[2], wr[2 * kDirHidden + n], fmaf(dv[1], wr[kDirHidden + n], dv[0] * wr[n]));
      }
  __syncthreads();                    // mask rows, w_sigma and constants in LDS
  const float* cst = lds + kBoLdsConsts;
  const float* wsig = lds + kBoLdsWsig;
  float* grow = tile_row(grad, s, kGradRow);
  if (valid && h == 0) {
    grow[tile_col(kGradSigma)] = dsp;
#pragma unroll
    for (int c = 0; c < 3; ++c) grow[tile_col(kGradRgb) + c] = dv[c];
  }
  // d hd rows; d pre_dir = d hd [r_dir > 0] (hd = ReLU(dir pre) + appearance): rows, max, split at
  // the exact maximum into operands 8..15 (the dir layer's 8 k-steps)
  Operand in[16];
  float m_dir = 0.0f;
  {
    const uint32_t* md = mwave + (lane & 31) * kMaskRow + (kMaskRDirByte + 8 * h) / 4;
    const uint32_t mk[2] = {md[0], md[1]};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 a, b;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = dhd[t][4 * q + e];
          b[e] = (mk[t / 2] >> (16 * (t % 2) + 4 * q + e)) & 1u ? a[e] : 0.0f;
          dhd[t][4 * q + e] = b[e];
          m_dir = fmaxf(m_dir, fabsf(b[e]));
        }
        if (store_dhd)   // (uniform; the training step's fused per-ray sums read none, param_grads)
          store16_rows<0>(a, ga.rows, ga.loff + 4u * (uint32_t)tile_col(kGradHd + 32 * t + 8 * q));
        store16_rows<0>(b, ga.rows, ga.loff + 4u * (uint32_t)tile_col(kGradDir + 32 * t + 8 * q));
      }
  }
  m_dir = sample_max(m_dir);
  // block exponent records (layout.h): lane j < 8 gathers entry j; [dpre_dir | dsigma_pre] is entry 7
  float bexp = 0.0f;
  {
    const float rec = block_exp_record(wave_max_nn(fmaxf(m_dir, fabsf(dsp))));
    bexp = (lane & 31) == 7 ? rec : bexp;
  }
  // Every split scale carries the sample's sign sgn (odd samples negative).  The MFMA unit's f32
  // accumulation of f16 products is not correctly rounded and its error leans negative (-0.12 ulp
  // on average, profiles/r04/mfma_f16_accumulation_rounding.log); a gradient row of an odd sample is
  // computed negated, so its rounding error comes back with the opposite sign, and the per-column
  // errors cancel in the sums over samples that make the weight and bias gradients instead of adding
  // up.  (Each row's own error is unchanged; the sign is exact: the scales stay powers of two.)
  const float sgn = (lane & 1) ? -1.0f : 1.0f;
  const float s_dir = sgn * pow2_scale(m_dir);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) split_into(dhd[t][4 * q + e] * s_dir, in[8 + 2 * t + q / 2], 4 * (q & 1) + e);
  // d pre_7's scale: |W_dh^T g + dsigma w_sigma| <= C_dir max|g| + |dsigma| max|w_sigma|
  float s_cur = sgn * pow2_scale(cst[kT16C + 7] * m_dir + fabsf(dsp) * cst[kT16WsigMax]);
  float inv_prev = cst[kT16InvS + 7] / s_dir;

  // the weight stream: W^T fragments of dir_linear's h-part, then trunk layers 7 .. 1
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_sched_barrier(0);
  const float* stream = packedT + kPackedT32Floats;
  const uint32_t lds_dma = (uint32_t)(uintptr_t)(lptr_t)lds + 1024u * wave;
  const uint32_t voff = 16u * lane + 1024u * wave;
  chunk_dma<0>(stream, 0, lds_dma, voff);
  chunk_dma<1>(stream, 1, lds_dma, voff);
  chunk_dma<2>(stream, 2, lds_dma, voff);
  wait_vmcnt<8>();
  __builtin_amdgcn_s_barrier();
  h16x8 a0[4][2], a1[4][2];
  read_kstep<0>(lds, a0, lane);
  f32x16 acc[8];
  float m = 0.0f;
  BwQuarter qv[2];
  using Yes = std::true_type;
  using No = std::false_type;

  // ---- dir layer: d h_7 = W_dh^T d pre_dir (8 k-steps, operands 8..15), 4 chunk-steps per group;
  // group B converts group A's tiles 0-3 (+ dsigma w_sigma, mask_7) into operands 0..7, two
  // quarters per half-step
  auto dir_operand = [&](auto i, auto kk) -> const Operand& { return in[8 + kstep_of(i, kk)]; };
  run_group<0, 4, 0, 3, kSideNone, true>(stream, 0, lds, lds_dma, voff, a0, a1, acc, lane, dir_operand, NoSide{});
  GradAt g_cur = ga, g_prev = ga;
  g_cur.slice = 7 * kHidden;
  g_cur.mlay = (kMaskLayerBytes / 4) * 7;
  run_group<1, 4, 0, 3, kSideHalf, true>(stream, 4, lds, lds_dma, voff, a0, a1, acc, lane, dir_operand,
                                         [&](auto i, auto kk, auto ph) __attribute__((always_inline)) {
                                           constexpr int hs = kstep_of(i, kk), P = decltype(ph)::value;
                                           bw_quarter<P, 0, 0, 2 * hs, true, true>(acc, inv_prev, dsp, wsig, h, s_cur,
                                                                                     in, m, qv[0], g_cur);
                                           bw_quarter<P, 0, 0, 2 * hs + 1, true, true>(acc, inv_prev, dsp, wsig, h,
                                                                                         s_cur, in, m, qv[1], g_cur);
                                         });

  // ---- trunk layers l = 7 .. 1: d h_{l-1} = W_l^T d pre_l.  On entry operands 0..7 hold d pre_l
  // tiles 0-3 split at s_cur, d h_l tiles 4-7 wait in acc[4..7] (unscaled by inv_prev), m holds the
  // max of d pre_l tiles 0-3.  Side-work schedule: mlp16_kernel's (kSidePrev / kSideCur).
  auto act_operand = [&](auto i, auto kk) -> const Operand& { return in[kstep_of(i, kk)]; };
  // group A's side: d pre_l tiles 4-7 (SG: layer 7 adds dsigma w_sigma)
  auto side_prev = [&](auto i, auto kk, auto ph, auto sg_tag) __attribute__((always_inline)) {
    constexpr int hs = kstep_of(i, kk), P = decltype(ph)::value;
    constexpr bool sg = decltype(sg_tag)::value;
    if constexpr (hs == 0) {
      bw_quarter<P, 4, 8, 0, sg, true>(acc, inv_prev, dsp, wsig, h, s_cur, in, m, qv[0], g_prev);
      bw_quarter<P, 4, 8, 1, sg, true>(acc, inv_prev, dsp, wsig, h, s_cur, in, m, qv[1], g_prev);
    } else if constexpr (hs <= 14) {
      bw_quarter<P, 4, 8, hs + 1, sg, true>(acc, inv_prev, dsp, wsig, h, s_cur, in, m, qv[0], g_prev);
    }
  };
  float s_nxt = 0.0f, inv_cur = 0.0f;
  // group B's side: d pre_{l-1} tiles 0-3 (SP: split for the next layer; layer 0 has no consumer)
  auto side_cur = [&](auto i, auto kk, auto ph, auto sp_tag) __attribute__((always_inline)) {
    constexpr int hs = kstep_of(i, kk), P = decltype(ph)::value;
    constexpr bool sp = decltype(sp_tag)::value;
    if constexpr (hs >= 1 && hs <= 14) {
      bw_quarter<P, 0, 0, hs - 1, false, sp>(acc, inv_cur, 0.0f, wsig, h, s_nxt, in, m, qv[0], g_cur);
    } else if constexpr (hs == 15) {
      bw_quarter<P, 0, 0, 14, false, sp>(acc, inv_cur, 0.0f, wsig, h, s_nxt, in, m, qv[0], g_cur);
      bw_quarter<P, 0, 0, 15, false, sp>(acc, inv_cur, 0.0f, wsig, h, s_nxt, in, m, qv[1], g_cur);
    }
  };
  auto layer = [&](int l, auto sg_tag, auto last_tag) __attribute__((always_inline)) {
    constexpr bool last = decltype(last_tag)::value;
    const int c0 = 8 + (7 - l) * 16;
    g_prev.slice = l * kHidden;
    g_prev.mlay = (kMaskLayerBytes / 4) * l;
    g_cur.slice = (l - 1) * kHidden;
    g_cur.mlay = (kMaskLayerBytes / 4) * (l - 1);
    inv_cur = cst[kT16InvS + l - 1] / s_cur;
    run_group<0, 8, 0, 3, kSidePrev, true>(stream, c0, lds, lds_dma, voff, a0, a1, acc, lane, act_operand,
                                           [&](auto i, auto kk, auto ph) __attribute__((always_inline)) {
                                             side_prev(i, kk, ph, sg_tag);
                                           });
    // the inputs of this layer are complete: the scale of d pre_{l-1} from the bound
    m = sample_max(m);
    {   // m = the sample's max |d pre_l|: entry l - 1 (uniform over the wave)
      const float rec = block_exp_record(wave_max_nn(m));
      bexp = (lane & 31) == l - 1 ? rec : bexp;
    }
    s_nxt = sgn * pow2_scale(cst[kT16C + l - 1] * m);
    m = 0.0f;
    if constexpr (last) {
      run_group<1, 8, 0, 0, kSideCur, true>(stream, c0 + 8, lds, lds_dma, voff, a0, a1, acc, lane, act_operand,
                                            [&](auto i, auto kk, auto ph) __attribute__((always_inline)) {
                                              side_cur(i, kk, ph, No{});
                                            });
    } else {
      run_group<1, 8, 0, 3, kSideCur, true>(stream, c0 + 8, lds, lds_dma, voff, a0, a1, acc, lane, act_operand,
                                            [&](auto i, auto kk, auto ph) __attribute__((always_inline)) {
                                              side_cur(i, kk, ph, Yes{});
                                            });
    }
    inv_prev = inv_cur;
    s_cur = s_nxt;
  };
  layer(7, Yes{}, No{});
#pragma unroll 1
  for (int l = 6; l >= 2; --l) layer(l, No{}, No{});
  layer(1, No{}, Yes{});
  // d pre_0 tiles 4-7: exposed (no MFMA left to hide behind)
  g_prev.slice = 0;
  g_prev.mlay = 0;
  static_for<16>([&](auto qc) __attribute__((always_inline)) {
    constexpr int QG = decltype(qc)::value;
    bw_quarter<0, 4, 8, QG, false, false>(acc, inv_prev, 0.0f, wsig, h, 0.0f, in, m, qv[0], g_prev);
    bw_quarter<1, 4, 8, QG, false, false>(acc, inv_prev, 0.0f, wsig, h, 0.0f, in, m, qv[0], g_prev);
  });
  {   // m = the sample's max |d pre_0| (tiles 0-3 from layer 1's group B, 4-7 above): entry 8, read by
      // the split-f16 layer-0 / skip-PE pair (wgrad_pair16_kernel)
    const float rec = block_exp_record(wave_max_nn(sample_max(m)));
    bexp = (lane & 31) == 8 ? rec : bexp;
  }
  // the records: sample j's feature kMetaGradF (lane half 1 writes a 0 four pad floats on; tail lanes'
  // offsets lie outside the buffer range)
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(h == 0 && (lane & 31) < 9 ? bexp : 0.0f), ga.rows,
                                        (int)ga.loff + 4 * (int)(tile_col(kMetaGradF) + kMetaGradF % 8), 0, 0);
}

// store_dhd = false (nerf_train_backward on the fused path of param_grads): the mask-row kernel leaves
// the d hd columns of the gradient rows unwritten (nothing reads them there).
int launch_mlp_backward(const float* packed, const float* packedT, const float* save, const uint32_t* masks,
                        const float* sigma, const float* rgb, const float* dsigma, const float* drgb, int64_t M,
                        float* grad, hipStream_t s, bool store_dhd) {
  if (M == 0) return NERF_OK;
  // tile-major gradient rows: the last block's rows past M are zeros (layout.h); its tail lanes store nothing
  if (M % 32 && hipMemsetAsync(grad + (M / 32) * 32 * kGradRow, 0, (size_t)32 * kGradRow * 4, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "mlp backward: hipMemsetAsync failed");
  if (g_mlp_arith == NERF_ARITH_F16X3) {
    if (masks)
      hipLaunchKernelGGL(mlp_backward16_bound_kernel, dim3((unsigned)((M + 127) / 128)), dim3(256), 0, s, packed,
                         packedT, masks, sigma, rgb, dsigma, drgb, M, grad, (int)store_dhd);
    else
      hipLaunchKernelGGL(mlp_backward16_kernel, dim3((unsigned)((M + 127) / 128)), dim3(256), 0, s, packed,
                         packedT, save, sigma, rgb, dsigma, drgb, M, grad);
    return check_launch("mlp_backward16_kernel");
  }
  hipLaunchKernelGGL(mlp_backward_kernel, dim3((unsigned)((M + 127) / 128)), dim3(256), 0, s, packed, packedT, save,
                     sigma, rgb, dsigma, drgb, M, grad);
  return check_launch("mlp_backward_kernel");
}

}  // namespace nerf
