// Training path (BASELINE config 5): the C ABI of include/nerfmi_train.h over the
// stage files (composite_bwd.hip, mlp_backward.hip with the transposed packers, wgrad.hip, adam.hip; forward:
// mlp.hip, mlp16.hip).  Host code only: argument checks, the workspace carve and the host-side
// table keyed by workspace, param_grads (which weight gradient runs where, on two streams) and
// every extern "C" entry point of the training step, with and without an occupancy grid.
//
// Reference: src/train.py:13-207 — volume_render (perturb=True, coarse only: render.py:83-86
// ignores n_importance), MSE against the target rgb (:87), loss.backward(), Adam (:90-92).
#include <mutex>
#include <unordered_map>

#include "host_api.h"
#include "train_internal.h"

namespace nerf {

// param_grads' workspace: two streams' partial buffers (wgrad_stream_floats, wgrad_plan.h) + the ray-sum buffers
static size_t max_wgrad_floats(int64_t M) {
  return 2 * ((wgrad_stream_floats(M) + 63) & ~(size_t)63) + ray_sum_floats(M) + 64;
}

// Training workspace (each region 256-B aligned), M = B*N samples:
//   dirs (B,3) | z (B,N) | feat (B,256) | encd (B,32) | rgb (M,3) | sigma (M) | maps (B,4)
//   | dsigma (M) | drgb (M,3) | sq_err (B) | save (M,kSaveRow) | masks (M,kMaskRow) | grad (M,kGradRow)
//   | wgrad partials
// With an occupancy grid (save / masks / grad then hold the M_live <= M compact rows; rgb, sigma,
// dsigma, drgb stay dense) the tail follows: the live list (M int32), the classify block counts, and
// the compact sigma (M), rgb (3M), dsigma (M), drgb (3M).  The count lives in the caller's live_count.
struct TrainWs {
  float *dirs, *z, *feat, *encd, *rgb, *sigma, *maps, *dsigma, *drgb, *sq_err, *save;
  uint32_t* masks;
  float *grad, *wgrad;
  size_t wgrad_floats;   // of the wgrad region: param_grads' workspace
  int* live;             // the occupancy tail (null without a grid)
  uint32_t* blocks;
  float *sigma_live, *rgb_live, *dsigma_live, *drgb_live;
  // the part's dense sample set and where its composite backward writes
  CompositeSamples samples(int64_t B, int N) const { return dense_samples(rgb, sigma, z, B, N); }
  CompositeGrads grads() const { return {dsigma, drgb, nullptr, nullptr, 0}; }
};

// one sample set's regions, dirs .. grad (the hierarchical step carves two of them)
static void carve_part(Carver& c, int64_t B, int N, TrainWs& w) {
  const size_t b = (size_t)B, M = b * (size_t)N, MT = (size_t)tile_rows((int64_t)M);   // tile-major rows (layout.h)
  w.dirs = c.take<float>(b * 3 * 4);
  w.z = c.take<float>(b * N * 4);
  w.feat = c.take<float>(b * kRayFeat * 4);
  w.encd = c.take<float>(b * 32 * 4);
  w.rgb = c.take<float>(M * 3 * 4);
  w.sigma = c.take<float>(M * 4);
  w.maps = c.take<float>(b * 4 * 4);
  w.dsigma = c.take<float>(M * 4);
  w.drgb = c.take<float>(M * 3 * 4);
  w.sq_err = c.take<float>(b * 4);
  w.save = c.take<float>(MT * kSaveRow * 4);
  w.masks = c.take<uint32_t>(M * kMaskRow * 4);
  w.grad = c.take<float>(MT * kGradRow * 4);
  w.wgrad = nullptr;
  w.wgrad_floats = 0;
  w.live = nullptr;
  w.blocks = nullptr;
  w.sigma_live = w.rgb_live = w.dsigma_live = w.drgb_live = nullptr;
}

static size_t train_carve(int64_t B, int N, bool occ, void* base, TrainWs& w) {
  const size_t M = (size_t)B * (size_t)N;
  Carver c{(char*)base};
  carve_part(c, B, N, w);
  const size_t wg = c.at;
  w.wgrad = c.take<float>(max_wgrad_floats((int64_t)M) * 4);
  w.wgrad_floats = (c.at - wg) / 4;
  if (occ) {
    w.live = c.take<int>(M * 4);
    w.blocks = c.take<uint32_t>(occ_block_count_bytes((int64_t)M));
    w.sigma_live = c.take<float>(M * 4);
    w.rgb_live = c.take<float>(M * 12);
    w.dsigma_live = c.take<float>(M * 4);
    w.drgb_live = c.take<float>(M * 12);
  }
  return c.at;
}

// An entry point's carve (`need`: what train_carve / hier_carve returned) of the caller's workspace,
// refused when that is too small.
static int check_ws(const char* fn, int64_t B, size_t ws_bytes, size_t need) {
  if (B > 0 && ws_bytes < need)
    return set_error(NERF_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
  return NERF_OK;
}

// floats of state_dict tensor p (nerf_pack_weights order)
static size_t param_floats(int p) {
  if (p < 16) {
    const int L = p / 2;
    if (p % 2) return kHidden;
    return (size_t)kHidden * (L == 0 ? kPosEnc : L == kSkipLayer ? kHidden + kPosEnc : kHidden);
  }
  switch (p) {
    case P_SIGMA_W: return kHidden;
    case P_SIGMA_B: return 1;
    case P_DIR_W: return (size_t)kDirHidden * (kHidden + kDirEnc);
    case P_DIR_B: return kDirHidden;
    case P_APP_W: return (size_t)kDirHidden * kAppDim;
    case P_APP_B: return kDirHidden;
    case P_RGB_W: return 3 * kDirHidden;
    default: return 3;
  }
}
// ... and where tensor p starts in a second gradient set with every tensor at a 64-float boundary
// (p = P_COUNT: the floats of the whole set)
static size_t grad_set_offset(int p) {
  size_t n = 0;
  for (int q = 0; q < p; ++q) n += (param_floats(q) + 63) & ~(size_t)63;
  return n;
}

// The hierarchical step's workspace: the coarse sample set's regions as above (dirs, feat
// and encd serve both passes), then the fine set's ((B, Nf): z = z_fine, its own rgb .. grad rows; its
// per-ray regions are unused), then
//   w_c (B,N) | z_all (B,N+Nf) | merged_src (B,N+Nf) uint16 | the fine part's parameter gradients
//   (every tensor at a 64-float boundary) | its dapp (B,32) | wgrad partials, sized for the larger part
struct HierWs {
  TrainWs c, f;
  float *w_c, *z_all;
  uint16_t* src;
  float *grad2, *dapp2, *wgrad;
  size_t wgrad_floats;
  // the merged sample set; its backward adds to the coarse rows (the coarse composite's term is there)
  CompositeSamples merged(int64_t B, int N, int Nf) const {
    return merged_samples(c.rgb, c.sigma, f.rgb, f.sigma, src, z_all, B, N, Nf);
  }
  CompositeGrads merged_grads() const { return {c.dsigma, c.drgb, f.dsigma, f.drgb, 1}; }
};

static bool hier_shape_ok(int64_t B, int N, int Nf) {
  return B >= 0 && N >= 2 && N <= 256 && Nf >= 1 && Nf <= 1024 && B * (int64_t)N < ((int64_t)1 << 31) &&
         B * (int64_t)Nf < ((int64_t)1 << 31);
}

static size_t hier_carve(int64_t B, int N, int Nf, void* base, HierWs& h) {
  const size_t b = (size_t)B, T = (size_t)(N + Nf);
  Carver c{(char*)base};
  carve_part(c, B, N, h.c);
  carve_part(c, B, Nf, h.f);
  h.w_c = c.take<float>(b * N * 4);
  h.z_all = c.take<float>(b * T * 4);
  h.src = c.take<uint16_t>((b * T + 1) / 2 * 4);
  h.grad2 = c.take<float>(grad_set_offset(P_COUNT) * 4);
  h.dapp2 = c.take<float>(b * kAppDim * 4);
  const size_t wc = max_wgrad_floats((int64_t)b * N), wf = max_wgrad_floats((int64_t)b * Nf), wg = c.at;
  h.wgrad = c.take<float>((wc > wf ? wc : wf) * 4);
  h.wgrad_floats = (c.at - wg) / 4;
  return c.at;
}

// What the last forward on a workspace was (a small host-side table keyed by workspace address): the
// MLP arithmetic it ran under, which step it belonged to (dense, occupancy grid, hierarchical), and for
// nerf_train_occ_forward its M_live.  A backward picks the mask source from the arithmetic (the f32
// forward writes no mask rows), not from the setting in force at backward time; each backward refuses
// a workspace another step's forward wrote.
enum StepKind { kStepDense, kStepOcc, kStepHier };
struct ForwardRecord {
  int arith;
  StepKind kind;
  int64_t M_live;
};
static std::mutex g_ws_mu;
static std::unordered_map<const void*, ForwardRecord> g_ws_forward;
static void remember_forward(const void* ws, ForwardRecord r) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  if (g_ws_forward.size() > 4096) g_ws_forward.clear();
  g_ws_forward[ws] = r;
}
static bool last_forward(const void* ws, ForwardRecord& r) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  const auto it = g_ws_forward.find(ws);
  if (it == g_ws_forward.end()) return false;
  r = it->second;
  return true;
}
// ---- the background and opacity term (include/nerfmi_train.h "background")
// The _bg entries' additions.  Off (no alpha, no background, acc_weight 0): the original entry's calls.
struct BgLoss {
  const float* alpha;
  const float* bg;
  int64_t bg_rows;
  double acc_weight;
  bool off() const { return !alpha && bg_rows == 0 && acc_weight == 0.0; }
};

static int check_bg_loss(const char* fn, const BgLoss& o, int64_t B) {
  REQUIRE(o.bg_rows == 0 || o.bg_rows == 1 || o.bg_rows == B, "%s: bg_rows=%lld with B=%lld (0, 1 or B)", fn,
          (long long)o.bg_rows, (long long)B);
  REQUIRE(o.bg_rows == 0 || o.bg, "%s: null bg with bg_rows=%lld", fn, (long long)o.bg_rows);
  REQUIRE(o.acc_weight >= 0.0 && o.acc_weight <= 3.0e38, "%s: acc_weight=%g (>= 0)", fn, o.acc_weight);   // (NaN fails)
  return NERF_OK;
}

// Per-ray scratch of the head: the head of the sample set's gradient rows, which nothing holds until
// launch_mlp_backward writes them after the head (stream order).  Its 6 x roundup64(B) floats always
// fit: a set's rows are at least 32 x kGradRow floats and at least kGradRow per ray.
struct BgScratch {
  float *acc, *g_rgb, *g_acc, *sq_acc;
};
static BgScratch bg_scratch(float* grad_rows, int64_t B) {
  const size_t b = ((size_t)B + 63) & ~(size_t)63;
  return BgScratch{grad_rows, grad_rows + b, grad_rows + 4 * b, grad_rows + 5 * b};
}
static_assert(kGradRow >= 6 * 64, "the head's per-ray scratch fits in a ray's gradient rows");

// ---- the distortion term (include/nerfmi_train.h "distortion")
// The _dist entries' addition.  Off (weight 0): the _bg entry's calls.
struct DistLoss {
  double weight, near, far;
  bool off() const { return weight == 0.0; }
};

static int check_dist_loss(const char* fn, const DistLoss& d) {
  REQUIRE(d.weight >= 0.0 && d.weight <= 3.0e38, "%s: dist_weight=%g (>= 0)", fn, d.weight);   // (NaN fails)
  REQUIRE(d.off() || (d.far > d.near && d.far - d.near <= 1.7e308 && d.near >= -1.7e308),
          "%s: near=%g far=%g (finite, far > near) with dist_weight > 0", fn, d.near, d.far);
  return NERF_OK;
}

// Its scratch, behind the head's in the same gradient rows: the composite's weights (B,T), their gradient
// g_w (B,T) and the per-ray loss (B), each at a 64-float boundary.  `rows` is the number of samples whose
// gradient rows the set owns (whole 32-row tiles of kGradRow floats); null when that is too small.
struct DistScratch {
  float *weights, *g_w, *loss_rays;
};
static bool dist_scratch(float* grad_rows, int64_t rows, int64_t B, int T, DistScratch& t) {
  const size_t b = ((size_t)B + 63) & ~(size_t)63, bt = ((size_t)B * (size_t)T + 63) & ~(size_t)63;
  t.weights = grad_rows + 6 * b;
  t.g_w = t.weights + bt;
  t.loss_rays = t.g_w + bt;
  return 7 * b + 2 * bt <= (size_t)tile_rows(rows) * kGradRow;
}

// ---- what a backward entry was asked for, and the one head of all of them
// The form is the entry (plain, _bg, _dist): it fixes which loss floats and outputs the caller gave.  The
// options may all be off in any form; a plain entry's are.
enum LossForm { kLossPlain, kLossBg, kLossDist };
struct StepLoss {
  LossForm form;
  BgLoss bg;
  DistLoss dist;
  bool off() const { return bg.off() && dist.off(); }
};

static int check_step_loss(const char* fn, const StepLoss& spec, int64_t B) {
  if (spec.form != kLossPlain)
    if (int rc = check_bg_loss(fn, spec.bg, B)) return rc;
  return spec.form == kLossDist ? check_dist_loss(fn, spec.dist) : NERF_OK;
}

// The loss layout of every entry: term k (0 colour, 1 opacity, 2 distortion) of part p (0 fine or the only
// one, 1 coarse) of P parts is loss[k * P + p].  One part's slots: its loss floats (null for a term the form
// lacks), its rgb_final (nullable), the weight of its loss and the samples whose gradient rows it owns.
struct PartLoss {
  float *rgb, *acc, *dist, *rgb_final;
  double weight;
  int64_t rows;
};
static PartLoss part_loss(const StepLoss& spec, float* loss, int p, int P, float* rgb_final, double weight,
                          int64_t rows) {
  return PartLoss{loss + p, spec.form != kLossPlain ? loss + P + p : nullptr,
                  spec.form == kLossDist ? loss + 2 * P + p : nullptr, rgb_final, weight, rows};
}

static int zero_loss(const char* fn, float* slot, hipStream_t s) {   // (a null slot: the form lacks the term)
  if (slot && hipMemsetAsync(slot, 0, 4, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "%s: hipMemsetAsync failed", fn);
  return NERF_OK;
}

// The backward's head of one part: sample set `in` (its per-ray regions and gradient rows are w's), its
// gradients into `out`, its loss terms and rgb_final into `l`.  A term the form has and the options leave
// off reads 0.  Two paths, by the options:
//   all off: the composite backward of the MSE (train.py:87) and its mean, the original entries' calls and
//     bits; rgb_final is rgb_map.
//   any on: the composite once more for the opacity of the rows the forward left (its maps go to the set's
//     unused `maps` region), the per-ray loss and gradient (g_rgb, g_acc), the composite backward in its _acc
//     form, and the means.  With the distortion term on, the composite also leaves its weights in the
//     scratch, distortion_kernel turns them into the per-ray loss and g_w = weight dist.weight / B * dl/dw,
//     and the backward runs in its _w form with (g_rgb, g_acc, g_w).
static int loss_head(const char* fn, const TrainWs& w, const CompositeSamples& in, const CompositeGrads& out,
                     const float* rgb_map, const float* target, const StepLoss& spec, const PartLoss& l,
                     hipStream_t s) {
  const int64_t B = in.B;
  const BgLoss& o = spec.bg;
  const DistLoss& d = spec.dist;
  const bool dist = !d.off();
  int rc;
  if (!dist && (rc = zero_loss(fn, l.dist, s))) return rc;
  if (spec.off()) {
    const float scale = (float)(l.weight * (2.0 / (3.0 * (double)B)));
    if ((rc = launch_composite_backward(in, upstream_loss(rgb_map, target, scale, w.sq_err), nullptr, out, s)))
      return rc;
    if ((rc = launch_loss(w.sq_err, B, l.rgb, s))) return rc;
    if ((rc = zero_loss(fn, l.acc, s))) return rc;
    if (l.rgb_final && hipMemcpyAsync(l.rgb_final, rgb_map, (size_t)B * 12, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return set_error(NERF_ERR_HIP, "%s: rgb_final copy failed", fn);
    return NERF_OK;
  }
  const BgScratch t = bg_scratch(w.grad, B);
  const CompositeBg acc_only{nullptr, 0, __builtin_nanf(""), t.acc};
  CompositeAccGrad acc{t.g_acc, __builtin_nanf("")};
  DistScratch ds{};
  const int T = in.merged ? in.N + in.Nf : in.N;
  if (dist && !dist_scratch(w.grad, l.rows, B, T, ds))
    return set_error(NERF_ERR_WORKSPACE, "distortion: the scratch of B=%lld T=%d exceeds the gradient rows",
                     (long long)B, T);
  if ((rc = launch_composite(in, w.maps, w.maps + 3 * B, ds.weights, &acc_only, s))) return rc;
  if (dist) {
    if ((rc = launch_distortion(ds.weights, in.z, B, T, 1.0 / (d.far - d.near), l.weight * d.weight / (double)B,
                                ds.loss_rays, ds.g_w, s)))
      return rc;
    acc.g_w = ds.g_w;
  }
  if ((rc = launch_bg_loss(rgb_map, t.acc, target, o.alpha, o.bg_rows ? o.bg : nullptr, o.bg_rows > 1 ? 3 : 0,
                           (float)o.acc_weight, (float)(l.weight * 2.0 / (3.0 * (double)B)),
                           (float)(l.weight * 2.0 / (double)B), B, t.g_rgb, t.g_acc, w.sq_err, t.sq_acc, l.rgb_final,
                           s)))
    return rc;
  if ((rc = launch_composite_backward(in, upstream_grad(t.g_rgb, nullptr), &acc, out, s))) return rc;
  if ((rc = launch_loss(w.sq_err, B, l.rgb, s))) return rc;
  if ((rc = launch_loss_rays(t.sq_acc, B, l.acc, s))) return rc;
  return dist ? launch_loss_rays(ds.loss_rays, B, l.dist, s) : NERF_OK;
}
}  // namespace nerf

using namespace nerf;

extern "C" {

size_t nerf_packed_transposed_floats(void) { return kPackedTFloats; }

int nerf_pack_weights_transposed(const float* const* params, float* packedT, nerf_stream_t stream) {
  REQUIRE(params && packedT, "nerf_pack_weights_transposed: null pointer");
  for (int i = 0; i < P_COUNT; ++i) REQUIRE(params[i], "nerf_pack_weights_transposed: parameter %d is null", i);
  return launch_packT(params, packedT, (hipStream_t)stream);
}

int nerf_pack_weights_transposed_host(const float* const* params, float* packedT) {
  REQUIRE(params && packedT, "nerf_pack_weights_transposed_host: null pointer");
  for (int i = 0; i < P_COUNT; ++i) REQUIRE(params[i], "nerf_pack_weights_transposed_host: parameter %d is null", i);
  packT_host(params, packedT);
  return NERF_OK;
}

int nerf_ray_features_train(const float* packed, const float* dirs, int64_t R, const float* app, int64_t app_rows,
                            float* feat, float* enc_d, nerf_stream_t stream) {
  REQUIRE(R >= 0, "nerf_ray_features_train: R=%lld", (long long)R);
  REQUIRE(app_rows == 0 || app_rows == 1 || app_rows == R, "nerf_ray_features_train: app_rows=%lld with R=%lld",
          (long long)app_rows, (long long)R);
  REQUIRE(R == 0 || (packed && dirs && feat && enc_d && (app_rows == 0 || app)),
          "nerf_ray_features_train: null pointer");
  return launch_ray_features(packed, dirs, R, app, app_rows, feat, (hipStream_t)stream, enc_d);
}

int nerf_mlp_forward_train(const float* packed, const float* origins, const float* dirs, const float* z_vals,
                           int64_t R, int N, const float* ray_feat, const float* enc_d, float* rgb, float* sigma,
                           float* save, uint32_t* masks, nerf_stream_t stream) {
  REQUIRE(R >= 0 && N >= 1, "nerf_mlp_forward_train: R=%lld N=%d", (long long)R, N);
  REQUIRE(R == 0 || (packed && origins && dirs && z_vals && ray_feat && enc_d && rgb && sigma && save),
          "nerf_mlp_forward_train: null pointer");
  REQUIRE(R == 0 || masks || g_mlp_arith != NERF_ARITH_F16X3, "nerf_mlp_forward_train: masks required under f16x3");
  return launch_mlp(packed, origins, dirs, z_vals, R, N, ray_feat, rgb, sigma, nullptr, 0, (hipStream_t)stream, save,
                    enc_d, masks);
}

// The checks of the composite stage's entries, one per sample-set kind (`ptrs`: every pointer the entry
// requires is there)
static int check_dense_stage(const char* fn, int64_t B, int N, bool ptrs) {
  REQUIRE(B >= 0, "%s: B=%lld", fn, (long long)B);
  if (N < 1 || N > 4096) return set_error(NERF_ERR_UNSUPPORTED, "%s: N=%d (1..4096)", fn, N);
  REQUIRE(B == 0 || ptrs, "%s: null pointer", fn);
  return NERF_OK;
}
static int check_merged_stage(const char* fn, int64_t B, int N, int Nf, bool ptrs) {
  REQUIRE(B >= 0, "%s: B=%lld", fn, (long long)B);
  if (N < 1 || N > 256 || Nf < 1 || Nf > 1024)
    return set_error(NERF_ERR_UNSUPPORTED, "%s: N=%d (1..256) Nf=%d (1..1024)", fn, N, Nf);
  REQUIRE(B == 0 || ptrs, "%s: null pointer", fn);
  return NERF_OK;
}
// ... and the _grad entries of either kind: plain (acc null), _acc and _w
static int dense_stage_grad(const char* fn, const float* rgb, const float* sigma, const float* z_vals,
                            const float* grad_rgb_map, const float* grad_depth_map, int64_t B, int N, float* dsigma,
                            float* drgb, const CompositeAccGrad* acc, nerf_stream_t stream) {
  if (int rc = check_dense_stage(fn, B, N, rgb && sigma && z_vals && dsigma && drgb)) return rc;
  return launch_composite_backward(dense_samples(rgb, sigma, z_vals, B, N), upstream_grad(grad_rgb_map, grad_depth_map),
                                   acc, {dsigma, drgb, nullptr, nullptr, 0}, (hipStream_t)stream);
}
static int merged_stage_grad(const char* fn, const float* rgb_c, const float* sigma_c, const float* rgb_f,
                             const float* sigma_f, const uint16_t* src, const float* z_all, const float* grad_rgb_map,
                             const float* grad_depth_map, int64_t B, int N, int Nf, int accumulate_coarse,
                             float* dsigma_c, float* drgb_c, float* dsigma_f, float* drgb_f, const CompositeAccGrad* acc,
                             nerf_stream_t stream) {
  if (int rc = check_merged_stage(fn, B, N, Nf, rgb_c && sigma_c && rgb_f && sigma_f && src && z_all && dsigma_c &&
                                                    drgb_c && dsigma_f && drgb_f))
    return rc;
  return launch_composite_backward(merged_samples(rgb_c, sigma_c, rgb_f, sigma_f, src, z_all, B, N, Nf),
                                   upstream_grad(grad_rgb_map, grad_depth_map), acc,
                                   {dsigma_c, drgb_c, dsigma_f, drgb_f, accumulate_coarse}, (hipStream_t)stream);
}

int nerf_composite_backward(const float* rgb, const float* sigma, const float* z_vals, const float* rgb_map,
                            const float* target, int64_t B, int N, float scale, float* dsigma, float* drgb,
                            float* sq_err, nerf_stream_t stream) {
  if (int rc = check_dense_stage("nerf_composite_backward", B, N,
                                 rgb && sigma && z_vals && rgb_map && target && dsigma && drgb && sq_err))
    return rc;
  return launch_composite_backward(dense_samples(rgb, sigma, z_vals, B, N), upstream_loss(rgb_map, target, scale, sq_err),
                                   nullptr, {dsigma, drgb, nullptr, nullptr, 0}, (hipStream_t)stream);
}

int nerf_composite_backward_grad(const float* rgb, const float* sigma, const float* z_vals, const float* grad_rgb_map,
                                 const float* grad_depth_map, int64_t B, int N, float* dsigma, float* drgb,
                                 nerf_stream_t stream) {
  return dense_stage_grad("nerf_composite_backward_grad", rgb, sigma, z_vals, grad_rgb_map, grad_depth_map, B, N,
                          dsigma, drgb, nullptr, stream);
}

int nerf_mlp_backward(const float* packed, const float* packedT, const float* save, const uint32_t* masks,
                      const float* sigma, const float* rgb, const float* dsigma, const float* drgb, int64_t M,
                      float* grad, nerf_stream_t stream) {
  REQUIRE(M >= 0, "nerf_mlp_backward: M=%lld", (long long)M);
  REQUIRE(M == 0 || (packed && packedT && save && sigma && rgb && dsigma && drgb && grad),
          "nerf_mlp_backward: null pointer");
  return launch_mlp_backward(packed, packedT, save, masks, sigma, rgb, dsigma, drgb, M, grad, (hipStream_t)stream);
}

size_t nerf_wgrad_workspace_bytes(int64_t M, int N, int K) {
  if (M < 0 || N < 1 || K < 0) return 0;
  return wgrad_workspace_floats(M, N, K) * 4;
}

int nerf_wgrad(const float* a, int64_t lda, int N, const float* x, int64_t ldx, int K, int64_t x_div, int64_t M,
               float* out_w, float* out_b, int accumulate, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  REQUIRE(M >= 0 && M < ((int64_t)1 << 31) && N >= 1 && K >= 0 && x_div >= 0, "nerf_wgrad: M=%lld N=%d K=%d",
          (long long)M, N, K);
  REQUIRE(lda >= N && (K == 0 || ldx >= K), "nerf_wgrad: lda=%lld ldx=%lld", (long long)lda, (long long)ldx);
  REQUIRE(M == 0 || (a && (K == 0 || x) && (K == 0 || out_w) && workspace), "nerf_wgrad: null pointer");
  if (ws_bytes < wgrad_workspace_floats(M, N, K) * 4)
    return set_error(NERF_ERR_WORKSPACE, "nerf_wgrad: workspace %zu < %zu bytes", ws_bytes,
                     wgrad_workspace_floats(M, N, K) * 4);
  WgradGemm j;   // row-major operands, no block exponents
  j.a = a, j.lda = lda, j.N = N;
  j.x = x, j.ldx = ldx, j.K = K, j.x_div = x_div;
  j.M = M;
  j.out_w = out_w, j.ldo = K, j.out_b = out_b, j.accumulate = accumulate;
  return launch_wgrad(j, (float*)workspace, ws_bytes / 4, (hipStream_t)stream);
}

// Every parameter gradient of NeRF (+ the appearance rows) from the saved activations and the
// per-sample gradient rows; param_grads follows nerf_pack_weights' 24-pointer order.
//
// Two streams.  The GEMMs are independent (each reads its slices of the save and gradient rows and
// writes its own parameters), so they run on the caller's stream and on a second library stream,
// each with its own partial buffer: one launch's tail, the small reductions and the memory-bound
// ray sums overlap the other stream's GEMMs.  Every output is still written by one GEMM and one
// fixed-order reduction (deterministic).  The second stream forks from the caller's after
// everything queued there (the gradient rows) and the caller's stream waits for it at the end.
struct PgStreams {
  hipStream_t s2 = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
static int pg_streams(PgStreams** out) {
  static thread_local PgStreams per_dev[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return set_error(NERF_ERR_HIP, "param_grads: hipGetDevice");
  PgStreams& p = per_dev[dev];
  if (!p.s2) {
    if (hipStreamCreateWithFlags(&p.s2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&p.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p.join, hipEventDisableTiming) != hipSuccess)
      return set_error(NERF_ERR_HIP, "param_grads: stream/event creation failed");
  }
  *out = &p;
  return NERF_OK;
}

// Where the block exponents of gradient entry ja and save entry jx live (layout.h)
static H16Meta block_exps(const float* save, const float* grad, int ja, int jx) {
  H16Meta m;
  if (ja < 0 || jx < 0) return m;
  m.a = grad + tile_col(kMetaGradF) + 8 * ja + kMetaGradF % 8;
  m.a_stride = 32 * (int64_t)kGradRow;
  m.x = save + tile_col(kMetaSaveF) + 8 * jx + kMetaSaveF % 8;
  m.x_stride = 32 * (int64_t)kSaveRow;
  return m;
}

// The jobs, on streams sa / sb with partial buffers wa / wb (wfl floats each) and the ray-sum
// buffers at `rays` (N >= kRaySumMinN).
static int param_grads_jobs(const float* save, const float* grad, int64_t M, int N, const float* app, int64_t app_rows,
                            const float* packed, float* const* g, float* dapp, float* wa, float* wb, size_t wfl,
                            float* rays, hipStream_t sa, hipStream_t sb) {
  // save and grad are tile-major rows (layout.h): a slice starting at feature c is the same layout at
  // float offset tile_col(c).  The skip layer's [h3 | enc_x] runs as a 256 x 256 block (the whole-tile
  // kernel) plus the 63 PE columns, instead of one 256 x 319 GEMM on 128 x 128 tiles (416 -> ~300 us per
  // step).  Stream B: the K <= 64 GEMMs, layers 6-7 and the heads below.
  constexpr int kSkipK = kHidden + kPosEnc;
  static_assert(kSaveEncX == save_h(3) + kHidden, "the skip layer's input [h3 | enc_x] is contiguous in the save row");
  // the check and the launch of one job, on stream B (partials wb) or A
  auto run = [&](const WgradGemm& j, bool on_b) -> int {
    if (wgrad_workspace_floats(j.M, j.N, j.K) > wfl) return set_error(NERF_ERR_WORKSPACE, "param_grads: workspace");
    return launch_wgrad(j, on_b ? wb : wa, wfl, on_b ? sb : sa);
  };
  // n gradient columns from feature ga over K save columns from feature sx, every sample's
  auto rows_gemm = [&](int ga, int n, int sx, int K, float* out_w, int ldo, float* out_b) {
    WgradGemm j;
    j.a = grad + tile_col(ga), j.lda = kGradRow, j.N = n;
    j.x = save + tile_col(sx), j.ldx = kSaveRow, j.K = K;
    j.M = M;
    j.out_w = out_w, j.ldo = ldo, j.out_b = out_b;
    j.tiled = true;
    return j;
  };
  // trunk layer l >= 1: d pre_l over h_{l-1} (the skip layer: its h3 columns), both with block exponents
  auto trunk = [&](int l) {
    WgradGemm j = rows_gemm(l * kHidden, kHidden, save_h(l - 1), kHidden, g[2 * l], l == kSkipLayer ? kSkipK : kHidden,
                            g[2 * l + 1]);
    j.meta = block_exps(save, grad, l - 1, l - 1);
    return j;
  };
  // d pre_l over enc_x: layer 0's weight and bias, the skip layer's PE columns
  auto pe_cols = [&](int l) {
    return l == 0 ? rows_gemm(0, kHidden, kSaveEncX, kPosEnc, g[0], kPosEnc, g[1])
                  : rows_gemm(l * kHidden, kHidden, kSaveEncX, kPosEnc, g[2 * l] + kHidden, kSkipK, nullptr);
  };
  // the 128 columns of the row-major rows at src (per-ray or per-block gradient sums) over per-ray inputs
  auto sums_gemm = [&](const float* src, int64_t ld, int64_t rows, const float* x, int64_t ldx, int K, int64_t x_div) {
    WgradGemm j;
    j.a = src, j.lda = ld, j.N = kDirHidden;
    j.x = x, j.ldx = ldx, j.K = K, j.x_div = x_div;
    j.M = rows;
    return j;
  };
  int rc;
  // layer 0 and the skip layer's PE columns (both over enc_x): one launch of the split arithmetic's
  // pair kernel; under f32 two K = 63 jobs on the f32 GEMM like every other weight gradient
  const bool pe_pair = g_mlp_arith == NERF_ARITH_F16X3;
  rc = pe_pair ? launch_wgrad_pe_pair(save, grad, M, g[0], g[1], g[8], wb, wfl, sb) : run(pe_cols(0), true);
  if (rc) return rc;
  for (int l = 1; l < 8; ++l) {
    if ((rc = run(trunk(l), l >= 6))) return rc;
    if (l == kSkipLayer && !pe_pair && (rc = run(pe_cols(l), true))) return rc;
  }
  // fused per-ray sums (the split arithmetic's dir/density launch writes d pre_dir's 8-sample sums,
  // the rgb head's launch d hd's block sums; blocks of 32 samples lie on one ray): below, on stream B
  const bool fused = rays && fused_ray_sums(N);
  // the rgb head: the streaming kernel (3 rows); fused, with the per-ray sums below
  if (!fused && (rc = launch_wgrad_head3(grad + tile_col(kGradRgb), save + tile_col(kSaveHd), M, g[P_RGB_W], g[P_RGB_B], wa,
                                         wfl, sa)))
    return rc;
  static_assert(kGradSigma == kGradDir + kDirHidden, "the density head's gradient follows dir_linear's");
  // The appearance tail, last on stream B: appearance_projection's gradient over the d hd rows at src
  // (`rows` of them, leading dimension ld, `group` of them per ray; tiled: the gradient rows themselves)
  // with x = the ray's embedding row (broadcast when app_rows == 1; row-major), then d app.
  auto app_tail = [&](const float* src, int64_t ld, int64_t rows, int group, bool tiled) -> int {
    if (app_rows == 0) return NERF_OK;     // no appearance: the projection is unused (models.py:146)
    WgradGemm j = sums_gemm(src, ld, rows, app, kAppDim, kAppDim, app_rows == 1 ? 0 : group);
    j.out_w = g[P_APP_W], j.ldo = kAppDim, j.out_b = g[P_APP_B];
    j.tiled = tiled, j.x_tiled = !tiled;
    if (int rc = run(j, true)) return rc;
    if (!dapp) return NERF_OK;
    if (app_rows == 1) return launch_app_grad(g[P_APP_B], 1, 1, 1, packed, dapp, sb, false);
    return launch_app_grad(src, ld, app_rows, group, packed, dapp, sb, tiled);
  };
  if (rays) {
    // Rays of N >= 32 samples.  dir_linear's h7 columns and the density head (1 row over h7) run as
    // one 160 x 256 GEMM on the whole-tile kernel (5 row tiles) over a = the gradient columns from
    // d pre_dir on ([d pre_dir | d sigma | pad | d hd...]) and x = h7: rows 0..127 are dir_linear's
    // gradient (+ its bias column), row 128 the density head's, rows 129.. are dropped (h7 is read once).
    // dir_linear's PE_4(d) columns and the appearance projection take per-ray inputs: GEMMs over
    // per-ray (or per-block) gradient sums, which replace two M-row GEMMs: under the split arithmetic
    // with N % 32 == 0 the dir/density launch itself writes d pre_dir's 8-sample sums and the rgb
    // head's launch d hd's block sums from d rgb_pre; otherwise ray_sums_kernel reads the
    // 256 gradient columns of every sample.
    const int64_t B = M / N;
    float* S = rays;                                       // B x 256 (fused: S8, (M / 8) x 128)
    float* S_hd = S + ray_sum_a_floats(M);                 // fused: (M / 32) x 128
    float* E = S_hd + ray_sum_b_floats(M);                 // B x 32
    constexpr int kDirRows = 160;
    WgradGemm dir = rows_gemm(kGradDir, kDirRows, save_h(7), kHidden, g[P_DIR_W], kHidden + kDirEnc, g[P_DIR_B]);
    dir.split = WgradSplit{kDirHidden, g[P_SIGMA_W], kHidden, kHidden, g[P_SIGMA_B], kDirHidden + 1};
    dir.meta = block_exps(save, grad, 7, 7);
    dir.meta.a_cols = kDirHidden + 1;                      // d pre_dir, d sigma (rows 129.. are dropped)
    dir.sums = fused ? S : nullptr;
    if ((rc = run(dir, true))) return rc;
    if (fused) {
      const HeadSums hs{save, packed, N, S_hd, E};   // (rgb_linear's weight gradient + S_hd, E)
      if ((rc = launch_wgrad_head3(grad + tile_col(kGradRgb), save + tile_col(kSaveHd), M, g[P_RGB_W], g[P_RGB_B], wb, wfl,
                                   sb, &hs)))
        return rc;
    } else if ((rc = launch_ray_sums(grad, save, B, N, S, E, sb))) {
      return rc;
    }
    // dir_linear's PE_4(d) columns over the sums: fused, the M / 8 rows of 8-sample sums (row m: samples
    // 8m .. 8m+7, ray 8m / N) and d hd's M / 32 block sums; else one 256-column row per ray
    const int64_t s_ld = fused ? kDirHidden : 256, s_rows = fused ? M / 8 : B;
    WgradGemm enc = sums_gemm(S, s_ld, s_rows, E, 32, kDirEnc, fused ? N / 8 : 1);
    enc.out_w = g[P_DIR_W] + kHidden, enc.ldo = kHidden + kDirEnc;
    if ((rc = run(enc, true))) return rc;
    if (fused) return app_tail(S_hd, kDirHidden, M / 32, N / 32, false);
    return app_tail(S + kDirHidden, 256, B, 1, false);
  }
  // dir_linear (128 rows over [h7 | enc_d]) and the density head (1 row over h7) in one GEMM: the
  // gradient row holds [d pre_dir | d sigma], so rows 0..127 are dir_linear's gradient and row 128
  // (its first 256 columns and the bias column) the density head's: h7 is read once
  WgradGemm dir = rows_gemm(kGradDir, kDirHidden + 1, save_h(7), kHidden + kDirEnc, g[P_DIR_W], kHidden + kDirEnc,
                            g[P_DIR_B]);
  dir.split = WgradSplit{kDirHidden, g[P_SIGMA_W], kHidden, kHidden, g[P_SIGMA_B]};
  if ((rc = run(dir, true))) return rc;
  return app_tail(grad + tile_col(kGradHd), kGradRow, M, N, true);
}

static int param_grads(const float* save, const float* grad, int64_t M, int N, const float* app, int64_t app_rows,
                       const float* packed, float* const* g, float* dapp, float* ws, size_t ws_floats,
                       hipStream_t s) {
  const bool ray_path = N >= kRaySumMinN;
  const size_t rf = ray_path ? ray_sum_floats(M) : 0;
  if (ws_floats < rf + 64) return set_error(NERF_ERR_WORKSPACE, "param_grads: workspace");
  const size_t avail = (ws_floats - rf) & ~(size_t)63;   // partial buffers; the ray sums after them, aligned
  float* rays = ray_path ? ws + avail : nullptr;
  const size_t w1 = (wgrad_stream_floats(M) + 63) & ~(size_t)63;
  const bool two = avail >= 2 * w1;
  if (!two) return param_grads_jobs(save, grad, M, N, app, app_rows, packed, g, dapp, ws, ws, avail, rays, s, s);
  PgStreams* ps;
  int rc;
  if ((rc = pg_streams(&ps))) return rc;
  if (hipEventRecord(ps->fork, s) != hipSuccess || hipStreamWaitEvent(ps->s2, ps->fork, 0) != hipSuccess)
    return set_error(NERF_ERR_HIP, "param_grads: stream fork failed");
  rc = param_grads_jobs(save, grad, M, N, app, app_rows, packed, g, dapp, ws, ws + w1, w1, rays, s, ps->s2);
  // join even after a failed launch, so the caller's stream never runs ahead of queued work
  if (hipEventRecord(ps->join, ps->s2) != hipSuccess || hipStreamWaitEvent(s, ps->join, 0) != hipSuccess)
    return rc ? rc : set_error(NERF_ERR_HIP, "param_grads: stream join failed");
  return rc;
}

int nerf_param_grads(const float* save, const float* grad, int64_t M, int N, const float* app, int64_t app_rows,
                     const float* packed, float* const* param_grads_out, float* dapp, void* workspace,
                     size_t ws_bytes, nerf_stream_t stream) {
  REQUIRE(M >= 0 && M < ((int64_t)1 << 31) && N >= 1 && M % N == 0, "nerf_param_grads: M=%lld N=%d",
          (long long)M, N);
  REQUIRE(app_rows == 0 || app_rows == 1 || app_rows * N == M, "nerf_param_grads: app_rows=%lld", (long long)app_rows);
  REQUIRE(param_grads_out && packed && workspace && (M == 0 || (save && grad)) && (app_rows == 0 || app),
          "nerf_param_grads: null pointer");
  for (int i = 0; i < P_COUNT; ++i) REQUIRE(param_grads_out[i], "nerf_param_grads: gradient %d is null", i);
  if (M == 0) return NERF_OK;
  return param_grads(save, grad, M, N, app, app_rows, packed, param_grads_out, dapp, (float*)workspace, ws_bytes / 4,
                     (hipStream_t)stream);
}

size_t nerf_param_grads_workspace_bytes(int64_t M) { return M < 0 ? 0 : max_wgrad_floats(M) * 4; }

int nerf_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
              double beta2, double eps, int64_t step, nerf_stream_t stream) {
  REQUIRE(n >= 0 && step >= 1, "nerf_adam: n=%lld step=%lld", (long long)n, (long long)step);
  REQUIRE(n == 0 || (param && grad && exp_avg && exp_avg_sq), "nerf_adam: null pointer");
  return launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------ the training step
// Dense: nerf_train_forward, nerf_train_backward.  With an occupancy grid (include/nerfmi_train.h
// "training with an occupancy grid") three calls, because the library never
// synchronises and the live count has to reach the host once: sample (normalise, draw z, classify into
// the ascending live list; dead rows of sigma / rgb zero-filled), forward (ray features, the gathered
// forward writing COMPACT save / mask rows, the dense composite) and backward (dense composite
// backward + loss, gather of dsigma / drgb, the per-row MLP backward and weight gradients over M_live
// rows: the N = 1 route of param_grads, enc_d in every save row).  The pieces below are both variants'.
constexpr int64_t kOccMaxSamples = (int64_t)1 << 30;   // the live list's int32 indices (occupancy.hip)

// the shape checks of the occupancy entry points
static int check_occ_shape(const char* fn, int64_t B, int N) {
  REQUIRE(B >= 0, "%s: B=%lld", fn, (long long)B);
  if (N < 1 || N > 4096) return set_error(NERF_ERR_UNSUPPORTED, "%s: N=%d (1..4096)", fn, N);
  if (B * (int64_t)N > kOccMaxSamples)
    return set_error(NERF_ERR_UNSUPPORTED, "%s: %lld samples exceed the limit %lld", fn, (long long)B * N,
                     (long long)kOccMaxSamples);
  return NERF_OK;
}

// ... and what nerf_train_occ_forward / _backward check next (`what` names the refused part)
static int check_occ_step(const char* fn, const char* what, int64_t B, int N, int64_t M_live, int64_t app_rows) {
  if (int rc = check_occ_shape(fn, B, N)) return rc;
  REQUIRE(M_live >= 0 && M_live <= B * (int64_t)N, "%s: M_live=%lld with B*N=%lld", fn, (long long)M_live,
          (long long)(B * (int64_t)N));
  REQUIRE(app_rows >= 0, "%s: app_rows=%lld", fn, (long long)app_rows);
  if (app_rows > 1)
    return set_error(NERF_ERR_UNSUPPORTED, "%s: app_rows=%lld (0 or 1: no per-ray appearance rows)", fn,
                     (long long)app_rows);
  if (g_mlp_arith != NERF_ARITH_F16X3)
    return set_error(NERF_ERR_UNSUPPORTED, "%s: the gathered training %s is f16x3 only", fn, what);
  return NERF_OK;
}

// the pointer checks of both backward entry points
static int check_backward_ptrs(const char* fn, const float* packed, const float* packedT, const float* rgb_map,
                               const float* target, int64_t B, const float* app, int64_t app_rows,
                               float* const* param_grads_out, const float* loss, const void* workspace) {
  REQUIRE(packed && packedT && param_grads_out && loss && workspace && (B == 0 || (rgb_map && target)) &&
              (app_rows == 0 || app),
          "%s: null pointer", fn);
  for (int i = 0; i < P_COUNT; ++i) REQUIRE(param_grads_out[i], "%s: gradient %d is null", fn, i);
  return NERF_OK;
}

// the forward's tail: the composite (render.py:56-80) and the optional copy of z
static int forward_tail(const char* fn, const TrainWs& w, int64_t B, int N, float* rgb_map, float* depth_map,
                        float* weights_out, float* z_out, hipStream_t s) {
  if (int rc = launch_composite(w.samples(B, N), rgb_map, depth_map, weights_out, nullptr, s)) return rc;
  if (z_out && hipMemcpyAsync(z_out, w.z, (size_t)B * N * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "%s: z copy failed", fn);
  return NERF_OK;
}

// The forward of the dense step and the coarse pass of the hierarchical one, into sample set w: ray features,
// stratified positions, the MLP with saves.
static int coarse_forward(const float* packed, const float* rays_o, const float* rays_d, int64_t B, double near,
                          double far, int N, const float* t_vals, int perturb, const float* t_rand, uint64_t seed,
                          const float* app, int64_t app_rows, const TrainWs& w, hipStream_t s) {
  int rc;
  // the directions normalised (render.py:19) by the ray-feature kernel, which writes them to w.dirs
  if ((rc = launch_ray_features(packed, rays_d, B, app, app_rows, w.feat, s, w.encd, w.dirs))) return rc;
  if ((rc = launch_stratified(rays_o, w.dirs, B, (float)near, (float)(far - near), N, t_vals, perturb, t_rand, seed,
                              w.z, nullptr, s)))
    return rc;                                                                                          // :22
  return launch_mlp(packed, rays_o, w.dirs, w.z, B, N, w.feat, w.rgb, w.sigma, nullptr, 0, s, w.save, w.encd,
                    w.masks);                                                                           // :49
}

size_t nerf_train_workspace_bytes(int64_t B, int N) {
  if (B < 0 || N < 1) return 0;
  TrainWs w;
  return train_carve(B, N, false, nullptr, w);
}

size_t nerf_train_occ_workspace_bytes(int64_t B, int N) {
  if (B < 0 || N < 1 || N > 4096 || B * (int64_t)N > kOccMaxSamples) return 0;
  TrainWs w;
  return train_carve(B, N, true, nullptr, w);
}

int nerf_train_forward(const float* packed, const float* rays_o, const float* rays_d, int64_t B, double near,
                       double far, int N, const float* t_vals, int perturb, const float* t_rand, uint64_t seed,
                       const float* app, int64_t app_rows, float* rgb_map, float* depth_map, float* weights_out,
                       float* z_out, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  REQUIRE(B >= 0, "nerf_train_forward: B=%lld", (long long)B);
  if (N < 1 || N > 4096) return set_error(NERF_ERR_UNSUPPORTED, "nerf_train_forward: N=%d (1..4096)", N);
  REQUIRE(app_rows == 0 || app_rows == 1 || app_rows == B, "nerf_train_forward: app_rows=%lld with B=%lld",
          (long long)app_rows, (long long)B);
  if (B == 0) return NERF_OK;
  REQUIRE((int64_t)B * N < ((int64_t)1 << 31), "nerf_train_forward: B*N=%lld too large", (long long)B * N);
  REQUIRE(packed && rays_o && rays_d && t_vals && rgb_map && depth_map && workspace && (app_rows == 0 || app),
          "nerf_train_forward: null pointer");
  TrainWs w;
  int rc;
  if ((rc = check_ws("nerf_train_forward", B, ws_bytes, train_carve(B, N, false, workspace, w)))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = coarse_forward(packed, rays_o, rays_d, B, near, far, N, t_vals, perturb, t_rand, seed, app, app_rows, w, s)))
    return rc;
  remember_forward(workspace, {g_mlp_arith, kStepDense, 0});
  return forward_tail("nerf_train_forward", w, B, N, rgb_map, depth_map, weights_out, z_out, s);
}

// nerf_train_backward and its _bg and _dist forms (rgb_final: null in the plain form)
static int train_backward(const char* fn, const float* packed, const float* packedT, const float* rgb_map,
                          const float* target, int64_t B, int N, const float* app, int64_t app_rows,
                          float* const* param_grads_out, float* dapp, float* loss, void* workspace, size_t ws_bytes,
                          const StepLoss& spec, float* rgb_final, nerf_stream_t stream) {
  REQUIRE(B >= 0 && N >= 1 && N <= 4096, "%s: B=%lld N=%d", fn, (long long)B, N);
  REQUIRE(app_rows == 0 || app_rows == 1 || app_rows == B, "%s: app_rows=%lld", fn, (long long)app_rows);
  int rc;
  if ((rc = check_step_loss(fn, spec, B))) return rc;
  if ((rc = check_backward_ptrs(fn, packed, packedT, rgb_map, target, B, app, app_rows, param_grads_out, loss,
                                workspace)))
    return rc;
  if (B == 0) return NERF_OK;
  TrainWs w;
  if ((rc = check_ws(fn, B, ws_bytes, train_carve(B, N, false, workspace, w)))) return rc;
  hipStream_t s = (hipStream_t)stream;
  // the mask rows exist only when this workspace's forward ran under f16x3; the backward's kernels
  // follow the arithmetic in force now (an f16x3 backward after an f32 forward reads the ReLU masks
  // from the saved activations instead)
  ForwardRecord fwd;
  if (!last_forward(workspace, fwd) || fwd.kind != kStepDense)
    return set_error(NERF_ERR_BAD_ARG, "%s: no nerf_train_forward wrote this workspace", fn);
  const uint32_t* masks = fwd.arith == NERF_ARITH_F16X3 ? w.masks : nullptr;
  const int64_t M = B * N;
  if ((rc = loss_head(fn, w, w.samples(B, N), w.grads(), rgb_map, target, spec,
                      part_loss(spec, loss, 0, 1, rgb_final, 1.0, M), s)))
    return rc;
  if ((rc = launch_mlp_backward(packed, packedT, w.save, masks, w.sigma, w.rgb, w.dsigma, w.drgb, M, w.grad, s,
                                /*store_dhd=*/!fused_ray_sums(N))))
    return rc;
  return param_grads(w.save, w.grad, M, N, app, app_rows, packed, param_grads_out, dapp, w.wgrad, w.wgrad_floats, s);
}

int nerf_train_backward(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                        int64_t B, int N, const float* app, int64_t app_rows, float* const* param_grads_out,
                        float* dapp, float* loss, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  return train_backward("nerf_train_backward", packed, packedT, rgb_map, target, B, N, app, app_rows, param_grads_out,
                        dapp, loss, workspace, ws_bytes, StepLoss{kLossPlain, {}, {}}, nullptr, stream);
}

int nerf_train_backward_bg(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                           int64_t B, int N, const float* app, int64_t app_rows, float* const* param_grads_out,
                           float* dapp, float* loss, void* workspace, size_t ws_bytes, const float* alpha,
                           const float* bg, int64_t bg_rows, double acc_weight, float* rgb_final,
                           nerf_stream_t stream) {
  const StepLoss spec{kLossBg, {alpha, bg, bg_rows, acc_weight}, {}};
  return train_backward("nerf_train_backward_bg", packed, packedT, rgb_map, target, B, N, app, app_rows,
                        param_grads_out, dapp, loss, workspace, ws_bytes, spec, rgb_final, stream);
}

int nerf_train_backward_dist(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                             int64_t B, int N, const float* app, int64_t app_rows, float* const* param_grads_out,
                             float* dapp, float* loss, void* workspace, size_t ws_bytes, const float* alpha,
                             const float* bg, int64_t bg_rows, double acc_weight, float* rgb_final, double dist_weight,
                             double near, double far, nerf_stream_t stream) {
  const StepLoss spec{kLossDist, {alpha, bg, bg_rows, acc_weight}, {dist_weight, near, far}};
  return train_backward("nerf_train_backward_dist", packed, packedT, rgb_map, target, B, N, app, app_rows,
                        param_grads_out, dapp, loss, workspace, ws_bytes, spec, rgb_final, stream);
}

int nerf_train_occ_sample(const float* rays_o, const float* rays_d, int64_t B, double near, double far, int N,
                          const float* t_vals, int perturb, const float* t_rand, uint64_t seed, const uint32_t* bits,
                          int G, const float* lo, const float* inv, int32_t* live_count, void* workspace,
                          size_t ws_bytes, nerf_stream_t stream) {
  int rc;
  if ((rc = check_occ_shape("nerf_train_occ_sample", B, N))) return rc;
  REQUIRE(bits && lo && inv && live_count, "nerf_train_occ_sample: null pointer");
  REQUIRE(B == 0 || (rays_o && rays_d && t_vals && workspace), "nerf_train_occ_sample: null pointer");
  if (G < 1 || G > 1024) return set_error(NERF_ERR_UNSUPPORTED, "nerf_train_occ_sample: G=%d outside 1..1024", G);
  TrainWs w;
  if ((rc = check_ws("nerf_train_occ_sample", B, ws_bytes, train_carve(B, N, true, workspace, w)))) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((rc = launch_normalize(rays_d, B, w.dirs, s))) return rc;                                          // render.py:19
  if ((rc = launch_stratified(rays_o, w.dirs, B, (float)near, (float)(far - near), N, t_vals, perturb, t_rand, seed,
                              w.z, nullptr, s)))
    return rc;
  return launch_occ_classify(rays_o, w.dirs, w.z, B, N, bits, G, lo, inv, w.live, live_count, nullptr, w.sigma, w.rgb,
                             w.blocks, s);
}

int nerf_train_occ_forward(const float* packed, const float* rays_o, int64_t B, int N, int64_t M_live,
                           const float* app, int64_t app_rows, float* rgb_map, float* depth_map, float* weights_out,
                           float* z_out, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  int rc;
  if ((rc = check_occ_step("nerf_train_occ_forward", "forward", B, N, M_live, app_rows))) return rc;
  if (B == 0) return NERF_OK;
  REQUIRE(packed && rays_o && rgb_map && depth_map && workspace && (app_rows == 0 || app),
          "nerf_train_occ_forward: null pointer");
  TrainWs w;
  if ((rc = check_ws("nerf_train_occ_forward", B, ws_bytes, train_carve(B, N, true, workspace, w)))) return rc;
  hipStream_t s = (hipStream_t)stream;
  // w.dirs holds the normalised directions (nerf_train_occ_sample): the features from them as they are
  if ((rc = launch_ray_features(packed, w.dirs, B, app, app_rows, w.feat, s, w.encd, nullptr))) return rc;
  if ((rc = launch_mlp16_live(packed, rays_o, w.dirs, w.z, N, w.feat, w.encd, w.live, M_live, w.rgb, w.sigma, w.rgb_live,
                              w.sigma_live, w.save, w.masks, s)))
    return rc;
  remember_forward(workspace, {g_mlp_arith, kStepOcc, M_live});
  return forward_tail("nerf_train_occ_forward", w, B, N, rgb_map, depth_map, weights_out, z_out, s);
}

// nerf_train_occ_backward and its _bg and _dist forms.  The head runs on the zero-filled dense rows: a dead
// sample has weight 0.
static int train_occ_backward(const char* fn, const float* packed, const float* packedT, const float* rgb_map,
                              const float* target, int64_t B, int N, int64_t M_live, const float* app,
                              int64_t app_rows, float* const* param_grads_out, float* dapp, float* loss,
                              void* workspace, size_t ws_bytes, const StepLoss& spec, float* rgb_final,
                              nerf_stream_t stream) {
  int rc;
  if ((rc = check_occ_step(fn, "step", B, N, M_live, app_rows))) return rc;
  if ((rc = check_step_loss(fn, spec, B))) return rc;
  if ((rc = check_backward_ptrs(fn, packed, packedT, rgb_map, target, B, app, app_rows, param_grads_out, loss,
                                workspace)))
    return rc;
  if (B == 0) return NERF_OK;
  TrainWs w;
  if ((rc = check_ws(fn, B, ws_bytes, train_carve(B, N, true, workspace, w)))) return rc;
  ForwardRecord fwd;
  if (!last_forward(workspace, fwd) || fwd.kind != kStepOcc || fwd.M_live != M_live)
    return set_error(NERF_ERR_BAD_ARG, "%s: no nerf_train_occ_forward with M_live=%lld wrote this "
                     "workspace", fn, (long long)M_live);
  hipStream_t s = (hipStream_t)stream;
  if ((rc = loss_head(fn, w, w.samples(B, N), w.grads(), rgb_map, target, spec,
                      part_loss(spec, loss, 0, 1, rgb_final, 1.0, B * N), s)))
    return rc;
  if (M_live == 0) {   // every sample dead: sigma = 0 is a constant of the step, every gradient is zero
    for (int p = 0; p < P_COUNT; ++p)
      if (hipMemsetAsync(param_grads_out[p], 0, param_floats(p) * 4, s) != hipSuccess)
        return set_error(NERF_ERR_HIP, "%s: hipMemsetAsync failed", fn);
    if (dapp && app_rows && hipMemsetAsync(dapp, 0, (size_t)kAppDim * 4, s) != hipSuccess)
      return set_error(NERF_ERR_HIP, "%s: hipMemsetAsync failed", fn);
    return NERF_OK;
  }
  if ((rc = launch_occ_gather_grads(w.dsigma, w.drgb, w.live, M_live, w.dsigma_live, w.drgb_live, s))) return rc;
  if ((rc = launch_mlp_backward(packed, packedT, w.save, w.masks, w.sigma_live, w.rgb_live, w.dsigma_live,
                                w.drgb_live, M_live, w.grad, s, /*store_dhd=*/true)))
    return rc;
  return param_grads(w.save, w.grad, M_live, 1, app, app_rows, packed, param_grads_out, dapp, w.wgrad,
                     w.wgrad_floats, s);
}

int nerf_train_occ_backward(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                            int64_t B, int N, int64_t M_live, const float* app, int64_t app_rows,
                            float* const* param_grads_out, float* dapp, float* loss, void* workspace, size_t ws_bytes,
                            nerf_stream_t stream) {
  return train_occ_backward("nerf_train_occ_backward", packed, packedT, rgb_map, target, B, N, M_live, app, app_rows,
                            param_grads_out, dapp, loss, workspace, ws_bytes, StepLoss{kLossPlain, {}, {}}, nullptr,
                            stream);
}

int nerf_train_occ_backward_bg(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                               int64_t B, int N, int64_t M_live, const float* app, int64_t app_rows,
                               float* const* param_grads_out, float* dapp, float* loss, void* workspace,
                               size_t ws_bytes, const float* alpha, const float* bg, int64_t bg_rows,
                               double acc_weight, float* rgb_final, nerf_stream_t stream) {
  const StepLoss spec{kLossBg, {alpha, bg, bg_rows, acc_weight}, {}};
  return train_occ_backward("nerf_train_occ_backward_bg", packed, packedT, rgb_map, target, B, N, M_live, app, app_rows,
                            param_grads_out, dapp, loss, workspace, ws_bytes, spec, rgb_final, stream);
}

int nerf_train_occ_backward_dist(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                                 int64_t B, int N, int64_t M_live, const float* app, int64_t app_rows,
                                 float* const* param_grads_out, float* dapp, float* loss, void* workspace,
                                 size_t ws_bytes, const float* alpha, const float* bg, int64_t bg_rows,
                                 double acc_weight, float* rgb_final, double dist_weight, double near, double far,
                                 nerf_stream_t stream) {
  const StepLoss spec{kLossDist, {alpha, bg, bg_rows, acc_weight}, {dist_weight, near, far}};
  return train_occ_backward("nerf_train_occ_backward_dist", packed, packedT, rgb_map, target, B, N, M_live, app,
                            app_rows, param_grads_out, dapp, loss, workspace, ws_bytes, spec, rgb_final, stream);
}

// ------------------------------------------------------------- the hierarchical step
// One network, two sample sets: the coarse pass of nerf_train_forward on (B, N), the H1 resample of its
// weights (positions are constants of the step), the forward with saves on the Nf new samples, and the
// merged composite over N + Nf.  The backward sums the coarse composite's term (scaled by coarse_weight)
// and the merged composite's into the coarse rows, runs the data and weight gradients once per part,
// each with its own per-ray length, and adds the fine part's gradients to the coarse part's.
static int check_hier_shape(const char* fn, int64_t B, int N, int Nf) {
  REQUIRE(B >= 0, "%s: B=%lld", fn, (long long)B);
  if (N < 2 || N > 256 || Nf < 1 || Nf > 1024)
    return set_error(NERF_ERR_UNSUPPORTED, "%s: N=%d (2..256) Nf=%d (1..1024)", fn, N, Nf);
  REQUIRE(hier_shape_ok(B, N, Nf), "%s: B*N=%lld B*Nf=%lld too large", fn, (long long)B * N, (long long)B * Nf);
  return NERF_OK;
}

size_t nerf_train_hier_workspace_bytes(int64_t B, int N, int Nf) {
  if (!hier_shape_ok(B, N, Nf)) return 0;
  HierWs h;
  return hier_carve(B, N, Nf, nullptr, h);
}

int nerf_train_hier_forward(const float* packed, const float* rays_o, const float* rays_d, int64_t B, double near,
                            double far, int N, int Nf, const float* t_vals, const float* u_lin, int perturb,
                            const float* t_rand, const float* u_rand, uint64_t seed, const float* app,
                            int64_t app_rows, float* rgb_map, float* depth_map, float* weights_out, float* z_out,
                            float* coarse_rgb, float* coarse_depth, float* coarse_weights_out, void* workspace,
                            size_t ws_bytes, nerf_stream_t stream) {
  const char* fn = "nerf_train_hier_forward";
  int rc;
  if ((rc = check_hier_shape(fn, B, N, Nf))) return rc;
  REQUIRE(app_rows == 0 || app_rows == 1 || app_rows == B, "%s: app_rows=%lld with B=%lld", fn, (long long)app_rows,
          (long long)B);
  if (B == 0) return NERF_OK;
  REQUIRE(packed && rays_o && rays_d && t_vals && u_lin && rgb_map && depth_map && coarse_rgb && coarse_depth &&
              workspace && (app_rows == 0 || app),
          "%s: null pointer", fn);
  HierWs h;
  if ((rc = check_ws(fn, B, ws_bytes, hier_carve(B, N, Nf, workspace, h)))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const TrainWs &c = h.c, &f = h.f;
  if ((rc = coarse_forward(packed, rays_o, rays_d, B, near, far, N, t_vals, perturb, t_rand, seed, app, app_rows, c, s)))
    return rc;
  remember_forward(workspace, {g_mlp_arith, kStepHier, 0});
  float* wc = coarse_weights_out ? coarse_weights_out : h.w_c;
  if ((rc = launch_composite(c.samples(B, N), coarse_rgb, coarse_depth, wc, nullptr, s))) return rc;
  // the resample (the draws of nerf_render_rays at ray0 = 0), the Nf new samples, the merged composite
  if ((rc = launch_importance(nullptr, nullptr, c.z, wc, B, N, Nf, u_lin, u_rand, seed ^ 0x5DEECE66Dull, h.z_all, nullptr,
                              nullptr, nullptr, nullptr, nullptr, f.z, nullptr, s, h.src)))
    return rc;
  if ((rc = launch_mlp(packed, rays_o, c.dirs, f.z, B, Nf, c.feat, f.rgb, f.sigma, nullptr, 0, s, f.save, c.encd,
                       f.masks)))
    return rc;
  if ((rc = launch_composite(h.merged(B, N, Nf), rgb_map, depth_map, weights_out, nullptr, s))) return rc;
  if (z_out && hipMemcpyAsync(z_out, h.z_all, (size_t)B * (N + Nf) * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "%s: z copy failed", fn);
  return NERF_OK;
}

// nerf_train_hier_backward and its _bg and _dist forms (rgb_final, coarse_final: null in the plain form)
static int train_hier_backward(const char* fn, const float* packed, const float* packedT, const float* rgb_map,
                               const float* coarse_rgb, const float* target, int64_t B, int N, int Nf,
                               double coarse_weight, const float* app, int64_t app_rows,
                               float* const* param_grads_out, float* dapp, float* loss, void* workspace,
                               size_t ws_bytes, const StepLoss& spec, float* rgb_final, float* coarse_final,
                               nerf_stream_t stream) {
  int rc;
  if ((rc = check_hier_shape(fn, B, N, Nf))) return rc;
  if ((rc = check_step_loss(fn, spec, B))) return rc;
  REQUIRE(app_rows == 0 || app_rows == 1 || app_rows == B, "%s: app_rows=%lld", fn, (long long)app_rows);
  REQUIRE(coarse_weight >= 0.0 && coarse_weight <= 3.0e38, "%s: coarse_weight=%g", fn, coarse_weight);
  if ((rc = check_backward_ptrs(fn, packed, packedT, rgb_map, target, B, app, app_rows, param_grads_out, loss,
                                workspace)))
    return rc;
  REQUIRE(B == 0 || coarse_rgb, "%s: null pointer", fn);
  if (B == 0) return NERF_OK;
  HierWs h;
  if ((rc = check_ws(fn, B, ws_bytes, hier_carve(B, N, Nf, workspace, h)))) return rc;
  ForwardRecord fwd;
  if (!last_forward(workspace, fwd) || fwd.kind != kStepHier)
    return set_error(NERF_ERR_BAD_ARG, "%s: no nerf_train_hier_forward wrote this workspace", fn);
  hipStream_t s = (hipStream_t)stream;
  const TrainWs &c = h.c, &f = h.f;
  const bool f16 = fwd.arith == NERF_ARITH_F16X3;
  // The coarse part's head (scaled by coarse_weight), then the merged one's, which adds into the coarse rows;
  // both before the first launch_mlp_backward, which reads those rows and overwrites the heads' scratch.
  if ((rc = loss_head(fn, c, c.samples(B, N), c.grads(), coarse_rgb, target, spec,
                      part_loss(spec, loss, 1, 2, coarse_final, coarse_weight, B * N), s)))
    return rc;
  if ((rc = loss_head(fn, f, h.merged(B, N, Nf), h.merged_grads(), rgb_map, target, spec,
                      part_loss(spec, loss, 0, 2, rgb_final, 1.0, B * Nf), s)))
    return rc;
  // the fine part's gradients go to the workspace's second set
  float* g2[P_COUNT];
  for (int p = 0; p < P_COUNT; ++p) g2[p] = h.grad2 + grad_set_offset(p);
  if ((rc = launch_mlp_backward(packed, packedT, c.save, f16 ? c.masks : nullptr, c.sigma, c.rgb, c.dsigma, c.drgb, B * N,
                                c.grad, s, /*store_dhd=*/!fused_ray_sums(N))))
    return rc;
  if ((rc = param_grads(c.save, c.grad, B * N, N, app, app_rows, packed, param_grads_out, dapp, h.wgrad, h.wgrad_floats,
                        s)))
    return rc;
  if ((rc = launch_mlp_backward(packed, packedT, f.save, f16 ? f.masks : nullptr, f.sigma, f.rgb, f.dsigma, f.drgb,
                                B * Nf, f.grad, s, /*store_dhd=*/!fused_ray_sums(Nf))))
    return rc;
  if ((rc = param_grads(f.save, f.grad, B * Nf, Nf, app, app_rows, packed, g2, dapp ? h.dapp2 : nullptr, h.wgrad,
                        h.wgrad_floats, s)))
    return rc;
  // coarse + fine, one float add per element (the appearance projection is unused without appearance rows)
  float* dst[P_COUNT + 1];
  const float* src[P_COUNT + 1];
  size_t n[P_COUNT + 1];
  int count = 0;
  for (int p = 0; p < P_COUNT; ++p) {
    if (app_rows == 0 && (p == P_APP_W || p == P_APP_B)) continue;
    dst[count] = param_grads_out[p], src[count] = g2[p], n[count] = param_floats(p);
    ++count;
  }
  if (dapp && app_rows) dst[count] = dapp, src[count] = h.dapp2, n[count] = (size_t)app_rows * kAppDim, ++count;
  return launch_add_segments(dst, src, n, count, s);
}

int nerf_train_hier_backward(const float* packed, const float* packedT, const float* rgb_map, const float* coarse_rgb,
                             const float* target, int64_t B, int N, int Nf, double coarse_weight, const float* app,
                             int64_t app_rows, float* const* param_grads_out, float* dapp, float* loss,
                             void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  return train_hier_backward("nerf_train_hier_backward", packed, packedT, rgb_map, coarse_rgb, target, B, N, Nf,
                             coarse_weight, app, app_rows, param_grads_out, dapp, loss, workspace, ws_bytes,
                             StepLoss{kLossPlain, {}, {}}, nullptr, nullptr, stream);
}

int nerf_train_hier_backward_bg(const float* packed, const float* packedT, const float* rgb_map,
                                const float* coarse_rgb, const float* target, int64_t B, int N, int Nf,
                                double coarse_weight, const float* app, int64_t app_rows,
                                float* const* param_grads_out, float* dapp, float* loss, void* workspace,
                                size_t ws_bytes, const float* alpha, const float* bg, int64_t bg_rows,
                                double acc_weight, float* rgb_final, float* coarse_final, nerf_stream_t stream) {
  const StepLoss spec{kLossBg, {alpha, bg, bg_rows, acc_weight}, {}};
  return train_hier_backward("nerf_train_hier_backward_bg", packed, packedT, rgb_map, coarse_rgb, target, B, N, Nf,
                             coarse_weight, app, app_rows, param_grads_out, dapp, loss, workspace, ws_bytes, spec,
                             rgb_final, coarse_final, stream);
}

int nerf_train_hier_backward_dist(const float* packed, const float* packedT, const float* rgb_map,
                                  const float* coarse_rgb, const float* target, int64_t B, int N, int Nf,
                                  double coarse_weight, const float* app, int64_t app_rows,
                                  float* const* param_grads_out, float* dapp, float* loss, void* workspace,
                                  size_t ws_bytes, const float* alpha, const float* bg, int64_t bg_rows,
                                  double acc_weight, float* rgb_final, float* coarse_final, double dist_weight,
                                  double near, double far, nerf_stream_t stream) {
  const StepLoss spec{kLossDist, {alpha, bg, bg_rows, acc_weight}, {dist_weight, near, far}};
  return train_hier_backward("nerf_train_hier_backward_dist", packed, packedT, rgb_map, coarse_rgb, target, B, N, Nf,
                             coarse_weight, app, app_rows, param_grads_out, dapp, loss, workspace, ws_bytes, spec,
                             rgb_final, coarse_final, stream);
}

int nerf_distortion(const float* weights, const float* z_vals, int64_t B, int T, double near, double far, double scale,
                    float* loss_rays, float* g_w, nerf_stream_t stream) {
  REQUIRE(B >= 0, "nerf_distortion: B=%lld", (long long)B);
  if (T < 1 || T > 4096) return set_error(NERF_ERR_UNSUPPORTED, "nerf_distortion: T=%d (1..4096)", T);
  REQUIRE(far > near && far - near <= 1.7e308, "nerf_distortion: near=%g far=%g (finite, far > near)", near, far);
  REQUIRE(scale == scale && scale >= -1.7e308 && scale <= 1.7e308, "nerf_distortion: scale=%g", scale);
  REQUIRE(B == 0 || (weights && z_vals), "nerf_distortion: null pointer");
  return launch_distortion(weights, z_vals, B, T, 1.0 / (far - near), scale, loss_rays, g_w, (hipStream_t)stream);
}

int nerf_composite_backward_grad_w(const float* rgb, const float* sigma, const float* z_vals, const float* grad_rgb_map,
                                   const float* grad_depth_map, int64_t B, int N, float* dsigma, float* drgb,
                                   const float* g_acc, float bd, const float* g_w, nerf_stream_t stream) {
  const CompositeAccGrad acc{g_acc, bd, g_w};
  return dense_stage_grad("nerf_composite_backward_grad_w", rgb, sigma, z_vals, grad_rgb_map, grad_depth_map, B, N,
                          dsigma, drgb, &acc, stream);
}

int nerf_composite_merged_backward_w(const float* rgb_c, const float* sigma_c, const float* rgb_f, const float* sigma_f,
                                     const uint16_t* src, const float* z_all, const float* grad_rgb_map,
                                     const float* grad_depth_map, int64_t B, int N, int Nf, int accumulate_coarse,
                                     float* dsigma_c, float* drgb_c, float* dsigma_f, float* drgb_f, const float* g_acc,
                                     float bd, const float* g_w, nerf_stream_t stream) {
  const CompositeAccGrad acc{g_acc, bd, g_w};
  return merged_stage_grad("nerf_composite_merged_backward_w", rgb_c, sigma_c, rgb_f, sigma_f, src, z_all, grad_rgb_map,
                           grad_depth_map, B, N, Nf, accumulate_coarse, dsigma_c, drgb_c, dsigma_f, drgb_f, &acc, stream);
}

int nerf_composite_backward_grad_acc(const float* rgb, const float* sigma, const float* z_vals,
                                     const float* grad_rgb_map, const float* grad_depth_map, int64_t B, int N,
                                     float* dsigma, float* drgb, const float* g_acc, float bd, nerf_stream_t stream) {
  const CompositeAccGrad acc{g_acc, bd};
  return dense_stage_grad("nerf_composite_backward_grad_acc", rgb, sigma, z_vals, grad_rgb_map, grad_depth_map, B, N,
                          dsigma, drgb, &acc, stream);
}

int nerf_composite_merged_backward_acc(const float* rgb_c, const float* sigma_c, const float* rgb_f,
                                       const float* sigma_f, const uint16_t* src, const float* z_all,
                                       const float* grad_rgb_map, const float* grad_depth_map, int64_t B, int N, int Nf,
                                       int accumulate_coarse, float* dsigma_c, float* drgb_c, float* dsigma_f,
                                       float* drgb_f, const float* g_acc, float bd, nerf_stream_t stream) {
  const CompositeAccGrad acc{g_acc, bd};
  return merged_stage_grad("nerf_composite_merged_backward_acc", rgb_c, sigma_c, rgb_f, sigma_f, src, z_all, grad_rgb_map,
                           grad_depth_map, B, N, Nf, accumulate_coarse, dsigma_c, drgb_c, dsigma_f, drgb_f, &acc, stream);
}

int nerf_composite_merged_backward(const float* rgb_c, const float* sigma_c, const float* rgb_f, const float* sigma_f,
                                   const uint16_t* src, const float* z_all, const float* grad_rgb_map,
                                   const float* grad_depth_map, int64_t B, int N, int Nf, int accumulate_coarse,
                                   float* dsigma_c, float* drgb_c, float* dsigma_f, float* drgb_f,
                                   nerf_stream_t stream) {
  return merged_stage_grad("nerf_composite_merged_backward", rgb_c, sigma_c, rgb_f, sigma_f, src, z_all, grad_rgb_map,
                           grad_depth_map, B, N, Nf, accumulate_coarse, dsigma_c, drgb_c, dsigma_f, drgb_f, nullptr,
                           stream);
}

int nerf_sample_importance_src(const float* z_vals, const float* weights, int64_t B, int N, int Nf, const float* u_lin,
                               const float* u_rand, uint64_t seed, float* z_all, float* z_fine, uint16_t* merged_src,
                               nerf_stream_t stream) {
  if (int rc = check_merged_stage("nerf_sample_importance_src", B, N, Nf,
                                  z_vals && weights && u_lin && z_all && z_fine && merged_src))
    return rc;
  return launch_importance(nullptr, nullptr, z_vals, weights, B, N, Nf, u_lin, u_rand, seed, z_all, nullptr, nullptr,
                           nullptr, nullptr, nullptr, z_fine, nullptr, (hipStream_t)stream, merged_src);
}

int nerf_mlp_forward_train_live(const float* packed, const float* origins, const float* dirs, const float* z_vals,
                                int64_t R, int N, const float* ray_feat, const float* enc_d, const int32_t* live,
                                int64_t M_live, float* rgb, float* sigma, float* rgb_live, float* sigma_live,
                                float* save, uint32_t* masks, nerf_stream_t stream) {
  if (int rc = check_occ_shape("nerf_mlp_forward_train_live", R, N)) return rc;
  REQUIRE(M_live >= 0 && M_live <= R * (int64_t)N, "nerf_mlp_forward_train_live: M_live=%lld with R*N=%lld",
          (long long)M_live, (long long)(R * (int64_t)N));
  REQUIRE(M_live == 0 || (packed && origins && dirs && z_vals && ray_feat && enc_d && live && rgb && sigma &&
                          rgb_live && sigma_live && save && masks),
          "nerf_mlp_forward_train_live: null pointer");
  if (g_mlp_arith != NERF_ARITH_F16X3)
    return set_error(NERF_ERR_UNSUPPORTED, "nerf_mlp_forward_train_live: the gathered kernel is f16x3 only");
  return launch_mlp16_live(packed, origins, dirs, z_vals, N, ray_feat, enc_d, live, M_live, rgb, sigma, rgb_live,
                           sigma_live, save, masks, (hipStream_t)stream);
}

}  // extern "C"
