// Fused positional encoding -> NeRF MLP forward on split-f16 MFMA ("f16x3") with the training saves
// (R4-R6 + §8f-2; reference src/models.py:105-162, :14-47): the forward of nerf_mlp_forward_train /
// nerf_train_forward.  Since round 6 the render calls run mlp16s_kernel (mlp16s.hip: the same
// arithmetic and weight stream on v_mfma_f32_16x16x32_f16), so this kernel is instantiated with
// SAVE = true only; its SAVE = false branches (the round-5 render kernel) are not compiled into the
// library, and the DESIGN §4 measurements of that kernel come from the round-5 sources (git history).
//
// Arithmetic.  Every dense layer out^T = W . in^T runs on v_mfma_f32_32x32x16_f16 as
//     hi(W) hi(a) + hi(W) lo(a) + lo(W) hi(a)       (f32 accumulation)
// with x*s = hi + lo + O(2^-24 |x*s|), hi = f16(x*s), lo = f16(x*s - hi), and s a power of two:
// per layer for W (packed, layout.h) and per SAMPLE for the activations.  A power-of-two scale
// of a column of B scales that column of the product exactly, so the accumulator holds
// s_w * s_j * (W a) and one multiply by the exact inverse recovers it.  The dropped lo*lo term
// and the split residual are both O(2^-24): the result has fp32-level error
// (tests/test_gpu_parity.py::test_forward_accuracy_vs_float64 measures it against float64 next
// to the exact-f32 kernel in mlp.hip), at 3 x 32 MFMA cycles per 16-deep k-step instead of the
// f32 instruction's 8 x 64.
//
// Scales from a bound, not a max.  Layer L+1's inputs y_L are split at s = 2^(14-e) with
// R_L max|a_L| + B_L < 2^e, where max|a_L| is the sample's largest input of layer L and R_L
// (max row L1 norm of W_L) and B_L (max |bias|) are pack-time constants: |y_L| <= R_L max|a_L|
// + B_L rigorously, so nothing overflows f16, and the scale is known before y_L exists.  (A
// loose bound only moves the split's absolute error floor, 2^-25 of the scaled unit, further
// below the sample's largest value.)  That lets outputs be converted tile by tile while MFMAs run:
//
// Schedule.  One wave owns 32 samples and runs the whole network for them; a layer's output
// tiles are the next layer's B operands in place (layout.h), so activations never leave
// registers.  A trunk layer's 8 tiles run as two groups of 4 over all k-steps.  The VALU
// epilogue of group A's outputs (unscale + bias, ReLU, split into the next layer's operands
// 0..7) runs in the MFMA shadow of group B's last 8 k-steps (operands 0..7 are dead by then);
// group B's epilogue (operands 8..15) runs in the shadow of the next layer's group A first 8
// k-steps, which read operands 0..7.  Only the prologue (PE) and the colour head stay exposed.
//
// Weight stream.  At 5.3x the f32 rate one wave would need ~21 B/clk of weights from L2, so the
// 4 waves of a workgroup share the stream: each 16 KiB chunk (2 k-steps x 4 tiles x {hi, lo}) is
// DMA'd once per workgroup (global_load_lds_dwordx4, a quarter by each wave) into a 4-slot LDS
// ring three chunks ahead, published by a counted vmcnt wait + barrier, and read back by all
// four waves with ds_read_b128 interleaved between the MFMAs.
#include "common.h"
#include "pe_sin.h"
#include "stream16.h"

namespace nerf {

// ---- LDS: one __shared__ array (a second object can make hipcc drain the DMA before every
// ds_read).  [ring: 4 x 16 KiB][PE: 4 waves x 32 x 64][biases 8 x 256 | density_head w 256, b 4]
// [layer constants].  Every small vector the layers read sits here: an ordinary global load used
// while a DMA is in flight makes hipcc wait vmcnt(0), draining the stream.
constexpr int kLdsPe = 4 * kChunkFloats;
constexpr int kLdsBias = kLdsPe + kW16Waves * kPeSteps * 64;
constexpr int kLdsSigmaW = kLdsBias + 8 * kHidden;
constexpr int kLdsVecFloats = 8 * kHidden + kHidden + 4;    // kOffBias .. kOffSigmaB + 4, contiguous in `packed`
constexpr int kLdsConsts = kLdsBias + kLdsVecFloats;
constexpr int kLdsRgb = kLdsConsts + kS16Consts;             // rgb_linear weight (3 x 128) + bias (4)
constexpr int kLdsRgbFloats = 3 * kDirHidden + 4;
constexpr int kLdsFeat = kLdsRgb + kLdsRgbFloats;             // per wave: its ray's features (256)
constexpr int kLdsFloats = kLdsFeat + kW16Waves * kRayFeat;   // 111 KiB
// Training forward only: each wave's 32 ReLU-mask rows (layout.h kMaskRow words, 272 B per
// sample), accumulated by ds_or from the epilogue quarters and copied out at the end.
constexpr int kMaskWords = kMaskRow;                          // 68
constexpr int kLdsMask = kLdsFloats;
constexpr int kLdsFloatsSave = kLdsMask + kW16Waves * 32 * kMaskWords;   // 145 KiB
static_assert(kOffRgbB == kOffRgbW + 3 * kDirHidden && kLdsRgb % 4 == 0 && kLdsFeat % 4 == 0, "LDS vector layout");
static_assert(kOffSigmaW == kOffBias + 8 * kHidden && kOffSigmaB == kOffSigmaW + kHidden, "packed vector order");


// ---- epilogue pieces (the side work) ----------------------------------------------------------
// Quarter QG (0..15) of a 4-tile group = registers 4q..4q+3 (q = QG % 4) of output tile T0 + QG / 4
// -> elements 4(q & 1) .. +3 of the next layer's operand in[OP0 + QG / 2]:
//   y = acc*inv + bias, r = ReLU(y), op = split(r*s); m tracks max r; SIGMA adds ws . r to part.
// Phase 0 (load4) reads the quarter's bias (and density weights) from LDS into `qv`; phase 1
// (convert4) computes.
struct QuarterVec {
  f32x4 b, w;
};
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
struct SaveAt {      // training forward: where a layer's activations go (see convert4)
  __amdgpu_buffer_rsrc_t rows;   // the wave's 32 activation rows
  uint32_t loff;                 // this lane's byte offset in the wave's tile-major block: ((lane & 31) 8 + 4h) 4
  int hoff;                      // the layer's slice (floats), uniform
  bool valid;
  unsigned* mrow;                // this lane's mask words in LDS: the sample's row + 4h (words)
  int mlay;                      // the layer's words in the row: 8 * layer, uniform
};
// ReLU-mask bits of tile T (quarter q, element e -> bit 4q + e: neuron 32T + 8q + 4h + e) go to
// bits 16 (T % 2) of word T / 2 of the lane's 4-word (16-byte) slot of the layer: exactly the
// 128-bit mask the backward folds from the activations (mlp_backward.hip dgrad16), so it loads one slot.
// One ds_or per quarter: no register lives across quarters.
__device__ __forceinline__ void mask_or(const SaveAt& sv, int T, uint32_t bits) {
  __hip_atomic_fetch_or(sv.mrow + sv.mlay + T / 2, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// 16 bytes at byte offset voff + 4 * (hoff + c) of the wave's rows: a buffer store, so the lane's
// address stays one VGPR (store16_rows, common.h: the whole offset in the VGPR, soffset 0).
// (tile-major rows, layout.h: feature group c / 8 of the slice at hoff; c and hoff multiples of 8, so
// one store instruction writes the wave's 32 samples x 8 features, 1 KiB, contiguously)
__device__ __forceinline__ void save_store(const SaveAt& sv, int c, f32x4 v) {
  store16_rows<kRowStoreAux>(v, sv.rows, sv.loff + 4u * (uint32_t)tile_col(sv.hoff) + 4u * (uint32_t)tile_col(c));
}
template <int T0, int QG, bool SIGMA>
__device__ __forceinline__ void load4(const float* bias, const float* ws, int h, QuarterVec& qv) {
  constexpr int T = T0 + QG / 4, q = QG % 4;
  qv.b = *reinterpret_cast<const f32x4*>(bias + 32 * T + 8 * q + 4 * h);
  if constexpr (SIGMA) qv.w = *reinterpret_cast<const f32x4*>(ws + 32 * T + 8 * q + 4 * h);
}
// SV (training forward): also store ReLU(y) to the sample's activation row (SaveAt): neuron
// 32T + 8q + 4h + e of the layer's slice, the layout.h save order.
template <int T0, int OP0, int QG, bool SIGMA, bool SV>
__device__ __forceinline__ void convert4(const f32x16 (&acc)[8], float inv, const QuarterVec& qv, float s,
                                         Operand (&in)[16], float& m, float& part, const SaveAt& sv) {
  constexpr int T = T0 + QG / 4, q = QG % 4;
  constexpr int SH = 16 * (T % 2) + 4 * q;
  f32x4 rv;
  float xs[4];
  uint32_t bits = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float r = fmaxf(fmaf(acc[T][4 * q + e], inv, qv.b[e]), 0.0f);
    rv[e] = r;
    m = fmaxf(m, r);
    if constexpr (SIGMA) part = fmaf(qv.w[e], r, part);
    xs[e] = r * s;
    if constexpr (SV) bits |= (r > 0.0f ? 1u : 0u) << (SH + e);
    else split_into(xs[e], in[OP0 + QG / 2], 4 * (q & 1) + e);
  }
  if constexpr (SV) {   // split: hi pairs by v_cvt_pk_f16_f32, lo pairs by split_lo_pair
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
  if constexpr (SV) {
    save_store(sv, 32 * T + 8 * q, rv);     // tail lanes: offset past the buffer, dropped
    mask_or(sv, T, bits);
  }
}
// Phase PH of quarter QG (slot J of this half-step's quarter vectors).
template <int PH, int T0, int OP0, int QG, bool SIGMA, bool SV>
__device__ __forceinline__ void quarter(const f32x16 (&acc)[8], float inv, const float* bias, const float* ws, int h,
                                        float s, Operand (&in)[16], float& m, float& part, QuarterVec& qv,
                                        const SaveAt& sv) {
  if constexpr (PH == 0) load4<T0, QG, SIGMA>(bias, ws, h, qv);
  else convert4<T0, OP0, QG, SIGMA, SV>(acc, inv, qv, s, in, m, part, sv);
}

// PE operand Q split at scale s from this wave's LDS copy (layer 4 reads [h3, enc_x]): phase 0
// reads the 8 values into `v`, phase 1 splits them.
template <int PH, int Q>
__device__ __forceinline__ void pe_operand(const float* pe_mine, float s, Operand& op, float (&v)[8], int lane) {
  if constexpr (PH == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = pe_mine[(8 * Q + j) * 64 + lane];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) split_into(v[j] * s, op, j);
  }
}


// SAVE = the training forward (nerf_mlp_forward_train): also writes each sample's activation row
// (layout.h kSave*: h_0..h_7 from the epilogue quarters, enc_x, enc_d, r_dir, hd from the heads)
// to `save` (M x kSaveRow); encd (R x 32) holds each ray's PE_4(d) from nerf_ray_features.
//
// The kernel, twice (mlp16_body.h): mlp16_kernel<SAVE> over the samples 0 .. M-1 of a launch, and
// mlp16_live_kernel, the training forward over the samples a live list names (training with an
// occupancy grid).  The body is included, not a template flag, so the dense kernel's
// preprocessed text, and with it its register allocation, is what it was.
#define MLP16_GATHER 0
#include "mlp16_body.h"
#undef MLP16_GATHER
#define MLP16_GATHER 1
#include "mlp16_body.h"
#undef MLP16_GATHER

int launch_mlp16(const float* packed, const float* o, const float* d, const float* z, int64_t R, int N,
                 const float* feat, float* rgb, float* sigma, const int* out_slot, int out_T, hipStream_t s,
                 float* save, const float* encd, uint32_t* masks) {
  const int64_t M = R * (int64_t)N;
  if (M == 0) return NERF_OK;
  constexpr int per_block = 32 * kW16Waves;
  const int64_t blocks = (M + per_block - 1) / per_block;
  if (save && !masks) return set_error(NERF_ERR_BAD_ARG, "mlp16 training forward: mask rows required");
  // tile-major save rows: the last block's rows past M are zeros (layout.h), its tail lanes store nothing
  if (save && M % 32 && hipMemsetAsync(save + (M / 32) * 32 * kSaveRow, 0, (size_t)32 * kSaveRow * 4, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "mlp16 training forward: hipMemsetAsync failed");
  if (!save) return launch_mlp16s(packed, o, d, z, R, N, feat, rgb, sigma, out_slot, out_T, s);
  hipLaunchKernelGGL(mlp16_kernel<true>, dim3((unsigned)blocks), dim3(64 * kW16Waves), 0, s, packed, o, d, z, M, N,
                     feat, rgb, sigma, out_slot, out_T, save, encd, masks);
  return check_launch("mlp16_kernel");
}

// The gathered training forward (nerf_mlp_forward_train_live, nerf_train_occ_forward): compact row i
// is sample live[i], i < M_live (host value: the backward and the weight gradients size their
// launches from it too).  save / masks / rgb_live / sigma_live hold M_live compact rows, rgb / sigma
// the launch's R N dense rows, of which only the listed ones are written.
int launch_mlp16_live(const float* packed, const float* o, const float* d, const float* z, int N, const float* feat,
                      const float* encd, const int* live, int64_t M_live, float* rgb, float* sigma, float* rgb_live,
                      float* sigma_live, float* save, uint32_t* masks, hipStream_t s) {
  const int64_t M = M_live;
  if (M == 0) return NERF_OK;
  constexpr int per_block = 32 * kW16Waves;
  const int64_t blocks = (M + per_block - 1) / per_block;
  if (M % 32 && hipMemsetAsync(save + (M / 32) * 32 * kSaveRow, 0, (size_t)32 * kSaveRow * 4, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "mlp16 gathered training forward: hipMemsetAsync failed");
  hipLaunchKernelGGL(mlp16_live_kernel, dim3((unsigned)blocks), dim3(64 * kW16Waves), 0, s, packed, o, d, z, M, N, feat,
                     rgb, sigma, live, rgb_live, sigma_live, save, encd, masks);
  return check_launch("mlp16_live_kernel");
}

}  // namespace nerf
