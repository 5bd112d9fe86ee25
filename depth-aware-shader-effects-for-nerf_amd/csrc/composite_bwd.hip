// Training path, stage 1 of the backward (BASELINE config 5): the composite
// backward.  Reference: src/train.py:77-92 (MSE against the target rgb :87, loss.backward())
// through src/render.py:56-80.
//
//   composite_backward_kernel   d loss / d(sigma, rgb) per sample from d loss / d rgb_map (and
//                               d depth_map), one wave per ray, reverse double-precision scan
//   composite_merged_backward_kernel   the same over the N + Nf merged samples of the hierarchical
//                               step, gathered from and written back to the coarse and fine rows
//                               through LDS
// Each also in an _acc form (a per-ray upstream gradient of the opacity, a background depth: DESIGN.md §15)
// and a _w form (the _acc form with a per-sample upstream gradient of the weights: DESIGN.md §16).
#include "composite_plan.h"
#include "train_internal.h"

namespace nerf {

// ---------------------------------------------------------------------------- composite bwd
// render.py:56-80 differentiated.  With g = d loss / d rgb_map (3), per sample s of a ray:
//   drgb_s = w_s g;  dw_s = g . rgb_s;  T_s = prod_{j<s} f_j, f_j = 1 - a_j + 1e-10
//   d a_s = dw_s T_s - (1/f_s) sum_{t>s} dw_t w_t;   d sigma_s = d a_s * dist_s * exp(-sigma_s dist_s)
// The training loss is mean((rgb_map - target)^2) over B x 3 (train.py:87): g = 2 (rgb_map - target)/(3B),
// sq_err[r] = sum_c (rgb_map - target)^2 for the loss value.  Given an arbitrary upstream gradient
// instead (autograd: grad_map (B,3) for rgb_map, grad_depth (B) for depth_map, each nullable = 0),
// g = grad_map[r] and the depth term of depth = S / (A + 1e-10), S = sum w z, A = sum w (:80) adds
//   dw_s += gd (z_s - S / (A + 1e-10)) / (A + 1e-10)
// with S and A re-accumulated in the forward pass.  dw, T, w and d a stay in double and d sigma is
// rounded once: d a_s is a difference of two terms of the size of dw (an empty sample in front of a
// surface: dw_s - sum dw_t w_t), and float roundings of dw, w and T there put d sigma twice as far from
// the float64 gradient as torch's fp32 autograd (tests/test_gpu_degenerate_rays.py).  drgb is the
// forward's float weight times g.

// ------------------------------------------------------------------- merged composite bwd
// The backward of composite.hip's MERGED composite (the hierarchical step): position
// p of ray r's T = N + Nf merged samples is sample e = src[r T + p] of cat[coarse, fine] (e < N: row
// r N + e of the coarse arrays, else row r Nf + e - N of the fine ones), z from z_all.  The
// arithmetic is composite_backward_kernel's, operation for operation and in its scan order (one
// wave per ray, 64 positions per chunk), so on the same merged rows the results are the same bits.
//
// Memory: the ray's coarse and fine (rgb, sigma) rows are first copied into LDS as one
// (r, g, b, sigma) quad per cat index with whole-row coalesced loads (the route of composite.hip's
// STAGE, which measured gathering from global memory at 6x the cost); the scans gather from there,
// write each sample's (drgb, dsigma) over the quad it came from (a cat index occurs once per ray,
// and a quad is last read when its sample's results are formed), and the quads go back to the split
// rows as whole coalesced rows.  Every output element has one writer.  Coarse rows take in + term
// when `accumulate` is set (the coarse composite's own term is already there), fine rows are always
// written.  LDS: 16 T bytes per ray; composite_plan.h puts 4 rays in a block up to T = 768 and 2 beyond
// (40 KB at its kMergedBwdMaxT).
constexpr int kMergedBwdChunks = kMergedBwdMaxT / 64;

#define COMPOSITE_BWD_ACC 0   // (the kernels, three times: composite_bwd_body.h)
#include "composite_bwd_body.h"
#undef COMPOSITE_BWD_ACC
#define COMPOSITE_BWD_ACC 1
#include "composite_bwd_body.h"
#undef COMPOSITE_BWD_W
#define COMPOSITE_BWD_W 1
#include "composite_bwd_body.h"
#undef COMPOSITE_BWD_W
#undef COMPOSITE_BWD_ACC

int launch_composite_backward(const CompositeSamples& in, const CompositeUpstream& up, const CompositeAccGrad* acc,
                              const CompositeGrads& out, hipStream_t s) {
  const bool per_sample = acc && acc->g_w;
  const CompositePlan p = composite_backward_plan(in.B, in.N, in.Nf, in.merged, acc != nullptr, per_sample);
  if (p.action == CompositePlan::kSkip) return NERF_OK;
  if (p.action == CompositePlan::kRefuse)
    return set_error(NERF_ERR_UNSUPPORTED, "composite_merged_backward: N=%d Nf=%d (N + Nf <= %d)", in.N, in.Nf,
                     kMergedBwdMaxT);
  const dim3 grid(p.grid), block(p.block);
  if (p.per_sample) {   // the _w kernels: the _acc arguments and g_w
    if (p.merged)
      hipLaunchKernelGGL(composite_merged_backward_w_kernel, grid, block, p.lds, s, in.rgb, in.sigma, in.rgb_f,
                         in.sigma_f, in.src, in.z, up.rgb_map, up.target, up.grad_map, up.grad_depth, in.B, in.N, in.Nf,
                         up.scale, out.accumulate, out.dsigma, out.drgb, out.dsigma_f, out.drgb_f, up.sq_err, acc->g_acc,
                         acc->bd, acc->g_w);
    else
      hipLaunchKernelGGL(composite_backward_w_kernel, grid, block, p.lds, s, in.rgb, in.sigma, in.z, up.rgb_map,
                         up.target, up.grad_map, up.grad_depth, in.B, in.N, up.scale, out.dsigma, out.drgb, up.sq_err,
                         acc->g_acc, acc->bd, acc->g_w);
    return check_launch(p.name);
  }
  switch (p.merged << 1 | p.alt) {
    case 0:
      hipLaunchKernelGGL(composite_backward_kernel, grid, block, p.lds, s, in.rgb, in.sigma, in.z, up.rgb_map, up.target,
                         up.grad_map, up.grad_depth, in.B, in.N, up.scale, out.dsigma, out.drgb, up.sq_err);
      break;
    case 1:
      hipLaunchKernelGGL(composite_backward_acc_kernel, grid, block, p.lds, s, in.rgb, in.sigma, in.z, up.rgb_map,
                         up.target, up.grad_map, up.grad_depth, in.B, in.N, up.scale, out.dsigma, out.drgb, up.sq_err,
                         acc->g_acc, acc->bd);
      break;
    case 2:
      hipLaunchKernelGGL(composite_merged_backward_kernel, grid, block, p.lds, s, in.rgb, in.sigma, in.rgb_f, in.sigma_f,
                         in.src, in.z, up.rgb_map, up.target, up.grad_map, up.grad_depth, in.B, in.N, in.Nf, up.scale,
                         out.accumulate, out.dsigma, out.drgb, out.dsigma_f, out.drgb_f, up.sq_err);
      break;
    case 3:
      hipLaunchKernelGGL(composite_merged_backward_acc_kernel, grid, block, p.lds, s, in.rgb, in.sigma, in.rgb_f,
                         in.sigma_f, in.src, in.z, up.rgb_map, up.target, up.grad_map, up.grad_depth, in.B, in.N, in.Nf,
                         up.scale, out.accumulate, out.dsigma, out.drgb, out.dsigma_f, out.drgb_f, up.sq_err, acc->g_acc,
                         acc->bd);
  }
  return check_launch(p.name);
}

// ------------------------------------------------------------- background loss
// The per-ray head of a training step with a background: one thread per ray, from the forward's
// rgb_map, the recomputed opacity acc, the target colour, its alpha (nullable = 1) and the background
// colour (bg null = black; stride 0: one colour, 3: one per ray), with k = max(0, 1 - acc):
//   target' = alpha target + (1 - alpha) bg      final = rgb_map + k bg   (composite_bg_kernel's blend)
//   g_rgb   = scale_rgb (final - target')        scale_rgb = 2 / (3B)
//   g_acc   = -(bg . g_rgb) where k > 0, else 0, + acc_weight scale_acc (acc - alpha), scale_acc = 2 / B
//   sq_rgb  = sum_c (final - target')^2          sq_acc = (acc - alpha)^2
// every product and sum rounded on its own.  Each output has one writer; the two means are reduced by
// loss_kernel / loss_rays_kernel (adam.hip) in their fixed order: deterministic, no float atomics.
__global__ void __launch_bounds__(256)
bg_loss_kernel(const float* __restrict__ rgb_map, const float* __restrict__ acc, const float* __restrict__ target,
               const float* __restrict__ alpha, const float* __restrict__ bg, int bg_stride, float acc_weight,
               float scale_rgb, float scale_acc, int64_t B, float* __restrict__ g_rgb, float* __restrict__ g_acc,
               float* __restrict__ sq_rgb, float* __restrict__ sq_acc, float* __restrict__ rgb_final) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= B) return;
  const float a = alpha ? alpha[r] : 1.0f;
  const float ac = acc[r];
  const float kb = fmaxf(0.0f, 1.0f - ac);
  const float ia = 1.0f - a;
  float dot = 0.0f, se = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float b = bg ? bg[(int64_t)bg_stride * r + c] : 0.0f;
    const float t1 = a * target[3 * r + c], t2 = ia * b;
    const float tp = t1 + t2;
    const float kbg = kb * b;
    const float fin = rgb_map[3 * r + c] + kbg;
    const float e = fin - tp;
    const float g = scale_rgb * e;
    const float ee = e * e, bgg = b * g;
    se = se + ee;
    dot = dot + bgg;
    g_rgb[3 * r + c] = g;
    if (rgb_final) rgb_final[3 * r + c] = fin;
  }
  const float ea = ac - a;
  const float ga_o = acc_weight * (scale_acc * ea);
  g_acc[r] = (kb > 0.0f ? -dot : 0.0f) + ga_o;
  sq_rgb[r] = se;
  sq_acc[r] = ea * ea;
}

int launch_bg_loss(const float* rgb_map, const float* acc, const float* target, const float* alpha, const float* bg,
                   int bg_stride, float acc_weight, float scale_rgb, float scale_acc, int64_t B, float* g_rgb,
                   float* g_acc, float* sq_rgb, float* sq_acc, float* rgb_final, hipStream_t s) {
  if (B == 0) return NERF_OK;
  hipLaunchKernelGGL(bg_loss_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, rgb_map, acc, target, alpha, bg,
                     bg_stride, acc_weight, scale_rgb, scale_acc, B, g_rgb, g_acc, sq_rgb, sq_acc, rgb_final);
  return check_launch("bg_loss_kernel");
}

// dst[i] += src[i] over up to 25 segments (the hierarchical step's second gradient set into the
// first): one writer per element, a single float add, so the sum has one fixed order
struct AddSegs {
  float* dst[25];
  const float* src[25];
  int n[25];
};
__global__ void __launch_bounds__(256) add_segments_kernel(AddSegs a) {
  const int seg = blockIdx.y;
  float* __restrict__ d = a.dst[seg];
  const float* __restrict__ x = a.src[seg];
  const int n = a.n[seg];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = d[i] + x[i];
}

int launch_add_segments(float* const* dst, const float* const* src, const size_t* n, int count, hipStream_t s) {
  if (count < 1 || count > 25) return set_error(NERF_ERR_BAD_ARG, "add_segments: count=%d", count);
  AddSegs a{};
  size_t most = 0;
  for (int i = 0; i < count; ++i) {
    a.dst[i] = dst[i], a.src[i] = src[i], a.n[i] = (int)n[i];
    most = n[i] > most ? n[i] : most;
  }
  if (most == 0) return NERF_OK;
  const unsigned gx = (unsigned)((most + 255) / 256 < 64 ? (most + 255) / 256 : 64);
  hipLaunchKernelGGL(add_segments_kernel, dim3(gx, (unsigned)count), dim3(256), 0, s, a);
  return check_launch("add_segments_kernel");
}

}  // namespace nerf
