// What crosses the training translation units (composite_bwd.hip, mlp_backward.hip, wgrad.hip,
// adam.hip, train_api.hip): the launchers' prototypes, the host structs passed between
// them, the weight gradients' job descriptor (their chunk policy and workspace sizers: wgrad_plan.h),
// and the f32 MFMA wrapper.  The transposed-weight layout is in layout.h; no kernel is defined here.
#pragma once
#include "common.h"
#include "wgrad_plan.h"

namespace nerf {

static_assert(kSaveRow == NERF_SAVE_ROW && kGradRow == NERF_GRAD_ROW, "nerfmi_train.h rows out of sync");

__device__ __forceinline__ f32x16 mfma32t(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------- weight gradient: chunks and workspace
// (the chunk policy, the workspace sizers and the route of a launch: wgrad_plan.h)
static_assert(kWgradArithF16x3 == NERF_ARITH_F16X3, "wgrad_plan.h's arithmetic out of sync");

struct H16Meta {                      // where the block exponents of a and x are (nullable: absent)
  const float* a = nullptr;           // record of block 0; block b at + b * a_stride
  int64_t a_stride = 0;
  const float* x = nullptr;
  int64_t x_stride = 0;
  int a_cols = 256;                   // a columns whose values count (the partial's kept rows)
};

struct WgradSplit {                  // rows n0 <= n < n_end of a weight gradient belong to a second parameter
  int n0 = 0;
  float* out_w = nullptr;            // its weight gradient, ld ldo, the first k columns
  int ldo = 0, k = 0;
  float* out_b = nullptr;            // its bias gradient (the bias column), nullable
  int n_end = 1 << 30;               // rows from n_end on are dropped (padding rows of a whole-tile launch)
};

// One weight-gradient GEMM (launch_wgrad): out_w[n][k] (ld ldo) and out_b[n] (nullable) (+)= sum over the M
// samples m of a[m][n] x[m / x_div][k] (x_div = 0: one broadcast x row) and of a[m][n].
struct WgradGemm {
  const float* a = nullptr; int64_t lda = 0; int N = 0;                     // M rows of N values, row length lda
  const float* x = nullptr; int64_t ldx = 0; int K = 0; int64_t x_div = 1;  // rows of K values, row length ldx
  int64_t M = 0;
  float* out_w = nullptr; int ldo = 0; float* out_b = nullptr; int accumulate = 0;
  WgradSplit split;                   // (out_w null: none)
  H16Meta meta;                       // the block exponents of a and x for the split-f16 whole-tile kernels (absent: none)
  // tiled: a (and x when x_div == 1 and x_tiled) are tile-major rows (layout.h) of row length lda / ldx,
  // each pointer at its slice's tile_col: the training path (param_grads).  Otherwise row-major.
  bool tiled = false, x_tiled = true;
  float* sums = nullptr;              // d pre_dir's 8-sample sums (wgrad_h16h_kernel's SUMS), nullable
};

// sums (nullable): S_hd and E of the fused per-ray sums (rays of N % 32 == 0 samples), save / packed
// the rows and weights they come from
struct HeadSums { const float* save; const float* packed; int N; float* S_hd; float* E; };

// The ray-sum buffers for any N >= kRaySumMinN (B = M / N <= M / kRaySumMinN rays): region A holds
// S (B x 256, ray_sums_kernel) or the fused path's 8-sample sums of d pre_dir ((M / 8) x 128), region
// B the fused path's S_hd ((M / 32) x 128), region C E (B x 32).
constexpr int kRaySumMinN = kEncDPerRayMinN;   // (enc_d per ray from there on, layout.h)
// The fused per-ray sums (the split arithmetic's dir/density launch writes d pre_dir's 8-sample sums,
// the rgb head's launch, wgrad_head3_kernel<true>, the rest): 32-sample blocks on one ray.  Then
// nothing reads d hd's columns.
inline bool fused_ray_sums(int N) { return g_mlp_arith == NERF_ARITH_F16X3 && N >= kRaySumMinN && N % 32 == 0; }
inline size_t ray_sum_a_floats(int64_t M) { return (size_t)(M / 8 + 1) * kDirHidden; }   // >= (M / 32 + 1) 256
inline size_t ray_sum_b_floats(int64_t M) { return (size_t)(M / 32 + 1) * kDirHidden; }
inline size_t ray_sum_floats(int64_t M) { return ray_sum_a_floats(M) + ray_sum_b_floats(M) + (size_t)(M / 32 + 1) * 32 + 64; }

// ------------------------------------------------------------------------------- launchers
// composite_bwd.hip: the composite backward over a sample set (CompositeSamples, common.h).
// The upstream gradient, one of two forms: the MSE against target (g = scale (rgb_map - target), sq_err (B)
// takes the squared errors), or given gradients of rgb_map (B,3) and depth_map (B), each nullable = 0.
struct CompositeUpstream {
  const float *rgb_map, *target;
  float scale;
  float* sq_err;
  const float *grad_map, *grad_depth;
};
inline CompositeUpstream upstream_loss(const float* rgb_map, const float* target, float scale, float* sq_err) {
  return {rgb_map, target, scale, sq_err, nullptr, nullptr};
}
inline CompositeUpstream upstream_grad(const float* grad_map, const float* grad_depth) {
  return {nullptr, nullptr, 0.0f, nullptr, grad_map, grad_depth};
}
// The opacity part (the _acc kernels: composite_bwd_body.h): g_acc (B, nullable = 0) is added
// to every dw of the ray; bd is the forward's background depth (NaN: the normalised depth).
// g_w ((B,N); merged: (B,N+Nf) in merged order; null: absent) is a per-sample gradient of the weights
// themselves, added to the sample's dw: non-null selects the _w kernels.
struct CompositeAccGrad {
  const float* g_acc;
  float bd;
  const float* g_w = nullptr;
};
// d loss / d(sigma, rgb) per sample; a merged set also has the fine pair, and its coarse rows take
// in + term when `accumulate` is set
struct CompositeGrads {
  float *dsigma, *drgb, *dsigma_f, *drgb_f;
  int accumulate;
};
// acc null: the plain kernels, else the _acc ones (with the gradient form of `up`), or the _w ones when
// acc->g_w is set
int launch_composite_backward(const CompositeSamples& in, const CompositeUpstream& up, const CompositeAccGrad* acc,
                              const CompositeGrads& out, hipStream_t s);
// distortion.hip: the distortion loss of the ray weights (include/nerfmi_train.h "distortion")
// over (B,T) weights and z, T in 1..4096: loss_rays (B) = (float)l_r and g_w (B,T) = (float)(scale dl_r/dw),
// each nullable; inv = 1 / (far - near)
int launch_distortion(const float* weights, const float* z, int64_t B, int T, double inv, double scale,
                      float* loss_rays, float* g_w, hipStream_t s);

// the per-ray loss head of a step with a background (composite_bwd.hip; the means: launch_loss / launch_loss_rays)
int launch_bg_loss(const float* rgb_map, const float* acc, const float* target, const float* alpha, const float* bg,
                   int bg_stride, float acc_weight, float scale_rgb, float scale_acc, int64_t B, float* g_rgb,
                   float* g_acc, float* sq_rgb, float* sq_acc, float* rgb_final, hipStream_t s);
// dst[k][i] += src[k][i], i < n[k], for count <= 25 segments in one launch
int launch_add_segments(float* const* dst, const float* const* src, const size_t* n, int count, hipStream_t s);
// mlp_backward.hip
int launch_packT(const float* const* params, float* packedT, hipStream_t s);
void packT_host(const float* const* params, float* packedT);
int launch_mlp_backward(const float* packed, const float* packedT, const float* save, const uint32_t* masks,
                        const float* sigma, const float* rgb, const float* dsigma, const float* drgb, int64_t M,
                        float* grad, hipStream_t s, bool store_dhd = true);
// wgrad.hip (the weight gradients)
int launch_wgrad(const WgradGemm& j, float* ws, size_t ws_floats, hipStream_t s);
int launch_wgrad_head3(const float* a, const float* x, int64_t M, float* out_w, float* out_b, float* ws,
                       size_t ws_floats, hipStream_t s, const HeadSums* sums = nullptr);
int launch_wgrad_pe_pair(const float* save, const float* grad, int64_t M, float* w0, float* b0, float* w4, float* ws,
                         size_t ws_floats, hipStream_t s);
int launch_app_grad(const float* src, int64_t ld, int64_t rows, int group, const float* packed, float* dapp,
                    hipStream_t s, bool tiled);
int launch_ray_sums(const float* grad, const float* save, int64_t B, int N, float* S, float* E, hipStream_t s);
// adam.hip
int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                double eps, int64_t step, hipStream_t s);
int launch_loss(const float* sq_err, int64_t B, float* loss, hipStream_t s);
int launch_loss_rays(const float* sq_err, int64_t B, float* loss, hipStream_t s);   // sum / B

}  // namespace nerf
