// Training path (BASELINE config 5): the C ABI of include/nerfmi_train.h over the
// stage files (composite_bwd.hip, mlp_backward.hip with the transposed packers, train.hip, adam.hip; forward:
// mlp.hip, mlp16.hip).  Host code only: argument checks, the workspace carves and the host-side
// tables keyed by workspace, param_grads (which weight gradient runs where, on two streams) and
// every extern "C" entry point of the training step, with and without an occupancy grid.
//
// Reference: src/train.py:13-207 — volume_render (perturb=True, coarse only: render.py:83-86
// ignores n_importance), MSE against the target rgb (:87), loss.backward(), Adam (:90-92).
#include <mutex>
#include <unordered_map>

#include "train_internal.h"

namespace nerf {

// Training workspace carve (each region 256-B aligned), M = B*N samples:
//   dirs (B,3) | z (B,N) | feat (B,256) | encd (B,32) | rgb (M,3) | sigma (M) | maps (B,4)
//   | dsigma (M) | drgb (M,3) | sq_err (B) | save (M,kSaveRow) | masks (M,kMaskRow) | grad (M,kGradRow)
//   | wgrad partials
enum { T_DIRS, T_Z, T_FEAT, T_ENCD, T_RGB, T_SIG, T_MAPS, T_DSIG, T_DRGB, T_SQE, T_SAVE, T_MASK, T_GRAD, T_WG,
       T_COUNT };

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the largest wgrad partial buffer over the parameter list of param_grads (one stream's)
static size_t wgrad_stream_floats(int64_t M) {
  const int Ks[] = {kPosEnc, kHidden, kHidden + kPosEnc, kHidden + kDirEnc, kAppDim, kDirHidden};
  size_t m = 0;
  for (int K : Ks) {
    const size_t f = wgrad_workspace_floats(M, kHidden, K);
    if (f > m) m = f;
  }
  return m;
}
// param_grads' workspace: two streams' partial buffers + the ray-sum buffers
static size_t max_wgrad_floats(int64_t M) {
  return 2 * ((wgrad_stream_floats(M) + 63) & ~(size_t)63) + ray_sum_floats(M) + 64;
}

// Which MLP arithmetic the last nerf_train_forward on a workspace ran under (the f32 forward writes no
// mask rows): nerf_train_backward picks the mask source from it, not from the setting in force at
// backward time.  A small host-side table keyed by workspace address.
static std::mutex g_ws_mu;
static std::unordered_map<const void*, int> g_ws_arith;
static void remember_forward_arith(const void* ws, int arith) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  if (g_ws_arith.size() > 4096) g_ws_arith.clear();
  g_ws_arith[ws] = arith;
}
static int forward_arith(const void* ws) {
  std::lock_guard<std::mutex> lk(g_ws_mu);
  const auto it = g_ws_arith.find(ws);
  return it == g_ws_arith.end() ? -1 : it->second;
}

static size_t train_carve(int64_t B, int N, size_t* off) {
  const size_t b = (size_t)B, M = b * (size_t)N, MT = (size_t)tile_rows((int64_t)M);   // tile-major rows (layout.h)
  const size_t sizes[T_COUNT] = {b * 3, b * N, b * kRayFeat, b * 32, M * 3, M, b * 4, M, M * 3, b,
                                 MT * kSaveRow, M * kMaskRow, MT * kGradRow, max_wgrad_floats((int64_t)M)};
  size_t at = 0;
  for (int i = 0; i < T_COUNT; ++i) {
    off[i] = at;
    at += align256(sizes[i] * 4);
  }
  return at;
}
}  // namespace nerf

using namespace nerf;

#define TREQUIRE(cond, ...)                                        \
  do {                                                             \
    if (!(cond)) return set_error(NERF_ERR_BAD_ARG, __VA_ARGS__);  \
  } while (0)

extern "C" {

size_t nerf_packed_transposed_floats(void) { return kPackedTFloats; }

int nerf_pack_weights_transposed(const float* const* params, float* packedT, nerf_stream_t stream) {
  TREQUIRE(params && packedT, "nerf_pack_weights_transposed: null pointer");
  for (int i = 0; i < P_COUNT; ++i) TREQUIRE(params[i], "nerf_pack_weights_transposed: parameter %d is null", i);
  return launch_packT(params, packedT, (hipStream_t)stream);
}

int nerf_pack_weights_transposed_host(const float* const* params, float* packedT) {
  TREQUIRE(params && packedT, "nerf_pack_weights_transposed_host: null pointer");
  for (int i = 0; i < P_COUNT; ++i) TREQUIRE(params[i], "nerf_pack_weights_transposed_host: parameter %d is null", i);
  packT_host(params, packedT);
  return NERF_OK;
}

int nerf_ray_features_train(const float* packed, const float* dirs, int64_t R, const float* app, int64_t app_rows,
                            float* feat, float* enc_d, nerf_stream_t stream) {
  TREQUIRE(R >= 0, "nerf_ray_features_train: R=%lld", (long long)R);
  TREQUIRE(app_rows == 0 || app_rows == 1 || app_rows == R, "nerf_ray_features_train: app_rows=%lld with R=%lld",
           (long long)app_rows, (long long)R);
  TREQUIRE(R == 0 || (packed && dirs && feat && enc_d && (app_rows == 0 || app)),
           "nerf_ray_features_train: null pointer");
  return launch_ray_features(packed, dirs, R, app, app_rows, feat, (hipStream_t)stream, enc_d);
}

int nerf_mlp_forward_train(const float* packed, const float* origins, const float* dirs, const float* z_vals,
                           int64_t R, int N, const float* ray_feat, const float* enc_d, float* rgb, float* sigma,
                           float* save, uint32_t* masks, nerf_stream_t stream) {
  TREQUIRE(R >= 0 && N >= 1, "nerf_mlp_forward_train: R=%lld N=%d", (long long)R, N);
  TREQUIRE(R == 0 || (packed && origins && dirs && z_vals && ray_feat && enc_d && rgb && sigma && save),
           "nerf_mlp_forward_train: null pointer");
  TREQUIRE(R == 0 || masks || g_mlp_arith != NERF_ARITH_F16X3, "nerf_mlp_forward_train: masks required under f16x3");
  return launch_mlp(packed, origins, dirs, z_vals, R, N, ray_feat, rgb, sigma, nullptr, 0, (hipStream_t)stream, save,
                    enc_d, masks);
}

int nerf_composite_backward(const float* rgb, const float* sigma, const float* z_vals, const float* rgb_map,
                            const float* target, int64_t B, int N, float scale, float* dsigma, float* drgb,
                            float* sq_err, nerf_stream_t stream) {
  TREQUIRE(B >= 0, "nerf_composite_backward: B=%lld", (long long)B);
  if (N < 1 || N > 4096) return set_error(NERF_ERR_UNSUPPORTED, "nerf_composite_backward: N=%d (1..4096)", N);
  TREQUIRE(B == 0 || (rgb && sigma && z_vals && rgb_map && target && dsigma && drgb && sq_err),
           "nerf_composite_backward: null pointer");
  return launch_composite_backward(rgb, sigma, z_vals, rgb_map, target, nullptr, nullptr, B, N, scale, dsigma, drgb,
                                   sq_err, (hipStream_t)stream);
}

int nerf_composite_backward_grad(const float* rgb, const float* sigma, const float* z_vals, const float* grad_rgb_map,
                                 const float* grad_depth_map, int64_t B, int N, float* dsigma, float* drgb,
                                 nerf_stream_t stream) {
  TREQUIRE(B >= 0, "nerf_composite_backward_grad: B=%lld", (long long)B);
  if (N < 1 || N > 4096) return set_error(NERF_ERR_UNSUPPORTED, "nerf_composite_backward_grad: N=%d (1..4096)", N);
  TREQUIRE(B == 0 || (rgb && sigma && z_vals && dsigma && drgb), "nerf_composite_backward_grad: null pointer");
  return launch_composite_backward(rgb, sigma, z_vals, nullptr, nullptr, grad_rgb_map, grad_depth_map, B, N, 0.0f,
                                   dsigma, drgb, nullptr, (hipStream_t)stream);
}

int nerf_mlp_backward(const float* packed, const float* packedT, const float* save, const uint32_t* masks,
                      const float* sigma, const float* rgb, const float* dsigma, const float* drgb, int64_t M,
                      float* grad, nerf_stream_t stream) {
  TREQUIRE(M >= 0, "nerf_mlp_backward: M=%lld", (long long)M);
  TREQUIRE(M == 0 || (packed && packedT && save && sigma && rgb && dsigma && drgb && grad),
           "nerf_mlp_backward: null pointer");
  return launch_mlp_backward(packed, packedT, save, masks, sigma, rgb, dsigma, drgb, M, grad, (hipStream_t)stream);
}

size_t nerf_wgrad_workspace_bytes(int64_t M, int N, int K) {
  if (M < 0 || N < 1 || K < 0) return 0;
  return wgrad_workspace_floats(M, N, K) * 4;
}

int nerf_wgrad(const float* a, int64_t lda, int N, const float* x, int64_t ldx, int K, int64_t x_div, int64_t M,
               float* out_w, float* out_b, int accumulate, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  TREQUIRE(M >= 0 && M < ((int64_t)1 << 31) && N >= 1 && K >= 0 && x_div >= 0, "nerf_wgrad: M=%lld N=%d K=%d",
           (long long)M, N, K);
  TREQUIRE(lda >= N && (K == 0 || ldx >= K), "nerf_wgrad: lda=%lld ldx=%lld", (long long)lda, (long long)ldx);
  TREQUIRE(M == 0 || (a && (K == 0 || x) && (K == 0 || out_w) && workspace), "nerf_wgrad: null pointer");
  if (ws_bytes < wgrad_workspace_floats(M, N, K) * 4)
    return set_error(NERF_ERR_WORKSPACE, "nerf_wgrad: workspace %zu < %zu bytes", ws_bytes,
                     wgrad_workspace_floats(M, N, K) * 4);
  return launch_wgrad(a, lda, N, x, ldx, K, x_div, M, out_w, K, out_b, accumulate, (float*)workspace,
                      (hipStream_t)stream);
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
  // Job: columns [k0, k0 + K) of parameter p's weight gradient (row length ldo) from x; the bias
  // gradient with the first column block only.  The skip layer's [h3 | enc_x] runs as a 256 x 256
  // block (the whole-tile kernel) plus the 63 PE columns, instead of one 256 x 319 GEMM on 128 x 128
  // tiles (416 -> ~300 us per step).
  // save and grad are tile-major rows (layout.h): a slice starting at feature c is the same layout at
  // float offset tile_col(c).  Stream B: the K <= 64 GEMMs, layers 6-7 and the heads below.
  // ja / jx: the block-exponent entries of a and x (layout.h; -1: none)
  struct Job { int a; int n; int x; int K; int p; int k0; int ldo; bool bias; bool b; int ja; int jx; };
  constexpr int kSkipK = kHidden + kPosEnc;
  const Job jobs[] = {
      {0, kHidden, kSaveEncX, kPosEnc, 0, 0, kPosEnc, true, true, -1, -1},
      {1 * kHidden, kHidden, save_h(0), kHidden, 2, 0, kHidden, true, false, 0, 0},
      {2 * kHidden, kHidden, save_h(1), kHidden, 4, 0, kHidden, true, false, 1, 1},
      {3 * kHidden, kHidden, save_h(2), kHidden, 6, 0, kHidden, true, false, 2, 2},
      {4 * kHidden, kHidden, save_h(3), kHidden, 8, 0, kSkipK, true, false, 3, 3},                  // h3 ..
      {4 * kHidden, kHidden, save_h(3) + kHidden, kPosEnc, 8, kHidden, kSkipK, false, true, -1, -1},  // .. | enc_x
      {5 * kHidden, kHidden, save_h(4), kHidden, 10, 0, kHidden, true, false, 4, 4},
      {6 * kHidden, kHidden, save_h(5), kHidden, 12, 0, kHidden, true, true, 5, 5},
      {7 * kHidden, kHidden, save_h(6), kHidden, 14, 0, kHidden, true, true, 6, 6},
      {kGradRgb, 3, kSaveHd, kDirHidden, P_RGB_W, 0, kDirHidden, true, false, -1, -1},
  };
  static_assert(kSaveEncX == save_h(3) + kHidden, "the skip layer's input [h3 | enc_x] is contiguous in the save row");
  int rc;
  // layer 0 and the skip layer's PE columns (both over enc_x): one launch of the split arithmetic's
  // pair kernel; under f32 two K = 63 jobs on the f32 GEMM like every other weight gradient
  const bool pe_pair = g_mlp_arith == NERF_ARITH_F16X3;
  if (pe_pair && (rc = launch_wgrad_pe_pair(save, grad, M, g[0], g[1], g[8], wb, wfl, sb))) return rc;
  // fused per-ray sums (the split arithmetic's dir/density launch writes d pre_dir's 8-sample sums,
  // the rgb head's launch d hd's block sums; blocks of 32 samples lie on one ray): below, on stream B
  const bool fused = rays && fused_ray_sums(N);
  for (const Job& j : jobs) {
    if (pe_pair && j.K == kPosEnc) continue;            // (in the pair above)
    if (fused && j.a == kGradRgb) continue;             // (with the per-ray sums below)
    if (wgrad_workspace_floats(M, j.n, j.K) > wfl) return set_error(NERF_ERR_WORKSPACE, "param_grads: workspace");
    if (j.a == kGradRgb) {   // the rgb head: the streaming kernel (3 rows)
      if ((rc = launch_wgrad_head3(grad + tile_col(kGradRgb), save + tile_col(kSaveHd), M, g[j.p], g[j.p + 1],
                                   j.b ? wb : wa, wfl, j.b ? sb : sa)))
        return rc;
      continue;
    }
    const H16Meta hm = block_exps(save, grad, j.ja, j.jx);
    if ((rc = launch_wgrad(grad + tile_col(j.a), kGradRow, j.n, save + tile_col(j.x), kSaveRow, j.K, 1, M, g[j.p] + j.k0,
                           j.ldo, j.bias ? g[j.p + 1] : nullptr, 0, j.b ? wb : wa, j.b ? sb : sa, nullptr, true, true,
                           j.ja >= 0 ? &hm : nullptr)))
      return rc;
  }
  static_assert(kGradSigma == kGradDir + kDirHidden, "the density head's gradient follows dir_linear's");
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
    if (wgrad_workspace_floats(M, kDirRows, kHidden) > wfl) return set_error(NERF_ERR_WORKSPACE, "param_grads: workspace");
    const WgradSplit heads{kDirHidden, g[P_SIGMA_W], kHidden, kHidden, g[P_SIGMA_B], kDirHidden + 1};
    H16Meta hm = block_exps(save, grad, 7, 7);
    hm.a_cols = kDirHidden + 1;                            // d pre_dir, d sigma (rows 129.. are dropped)
    if ((rc = launch_wgrad(grad + tile_col(kGradDir), kGradRow, kDirRows, save + tile_col(save_h(7)), kSaveRow, kHidden, 1,
                           M, g[P_DIR_W], kHidden + kDirEnc, g[P_DIR_B], 0, wb, sb, &heads, true, true, &hm,
                           fused ? S : nullptr)))
      return rc;
    if (fused) {
      const HeadSums hs{save, packed, N, S_hd, E};   // (rgb_linear's weight gradient + S_hd, E)
      if ((rc = launch_wgrad_head3(grad + tile_col(kGradRgb), save + tile_col(kSaveHd), M, g[P_RGB_W], g[P_RGB_B], wb, wfl,
                                   sb, &hs)))
        return rc;
      // dir_linear's PE_4(d) columns over the M / 8 rows of 8-sample sums (row m: samples 8m .. 8m+7,
      // ray 8m / N)
      if ((rc = launch_wgrad(S, kDirHidden, kDirHidden, E, 32, kDirEnc, N / 8, M / 8, g[P_DIR_W] + kHidden,
                             kHidden + kDirEnc, nullptr, 0, wb, sb)))
        return rc;
      if (app_rows == 0) return NERF_OK;     // no appearance: the projection is unused (models.py:146)
      if ((rc = launch_wgrad(S_hd, kDirHidden, kDirHidden, app, kAppDim, kAppDim, app_rows == 1 ? 0 : N / 32, M / 32,
                             g[P_APP_W], kAppDim, g[P_APP_B], 0, wb, sb)))
        return rc;
      if (!dapp) return NERF_OK;
      if (app_rows == 1) return launch_app_grad(g[P_APP_B], 1, 1, 1, packed, dapp, sb, false);
      return launch_app_grad(S_hd, kDirHidden, app_rows, N / 32, packed, dapp, sb, false);
    }
    if ((rc = launch_ray_sums(grad, save, B, N, S, E, sb))) return rc;
    if ((rc = launch_wgrad(S, 256, kDirHidden, E, 32, kDirEnc, 1, B, g[P_DIR_W] + kHidden, kHidden + kDirEnc, nullptr,
                           0, wb, sb)))
      return rc;
    if (app_rows == 0) return NERF_OK;     // no appearance: the projection is unused (models.py:146)
    if ((rc = launch_wgrad(S + kDirHidden, 256, kDirHidden, app, kAppDim, kAppDim, app_rows == 1 ? 0 : 1, B,
                           g[P_APP_W], kAppDim, g[P_APP_B], 0, wb, sb)))
      return rc;
    if (!dapp) return NERF_OK;
    if (app_rows == 1) return launch_app_grad(g[P_APP_B], 1, 1, 1, packed, dapp, sb, false);
    return launch_app_grad(S + kDirHidden, 256, app_rows, 1, packed, dapp, sb, false);
  }
  // dir_linear (128 rows over [h7 | enc_d]) and the density head (1 row over h7) in one GEMM: the
  // gradient row holds [d pre_dir | d sigma], so rows 0..127 are dir_linear's gradient and row 128
  // (its first 256 columns and the bias column) the density head's: h7 is read once
  if (wgrad_workspace_floats(M, kDirHidden + 1, kHidden + kDirEnc) > wfl)
    return set_error(NERF_ERR_WORKSPACE, "param_grads: workspace");
  const WgradSplit heads{kDirHidden, g[P_SIGMA_W], kHidden, kHidden, g[P_SIGMA_B]};
  if ((rc = launch_wgrad(grad + tile_col(kGradDir), kGradRow, kDirHidden + 1, save + tile_col(save_h(7)), kSaveRow,
                         kHidden + kDirEnc, 1, M, g[P_DIR_W], kHidden + kDirEnc, g[P_DIR_B], 0, wb, sb, &heads, true)))
    return rc;
  if (app_rows == 0) {   // no appearance: the projection is unused (models.py:146)
    return NERF_OK;
  }
  // appearance_projection: x = the ray's embedding row (broadcast when app_rows == 1; row-major)
  const int64_t xdiv = app_rows == 1 ? 0 : N;
  if ((rc = launch_wgrad(grad + tile_col(kGradHd), kGradRow, kDirHidden, app, kAppDim, kAppDim, xdiv, M, g[P_APP_W],
                         kAppDim, g[P_APP_B], 0, wb, sb, nullptr, true, /*x_tiled=*/false)))
    return rc;
  if (!dapp) return NERF_OK;
  if (app_rows == 1) return launch_app_grad(g[P_APP_B], 1, 1, 1, packed, dapp, sb, false);
  return launch_app_grad(grad + tile_col(kGradHd), kGradRow, app_rows, N, packed, dapp, sb, true);
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
  TREQUIRE(M >= 0 && M < ((int64_t)1 << 31) && N >= 1 && M % N == 0, "nerf_param_grads: M=%lld N=%d",
           (long long)M, N);
  TREQUIRE(app_rows == 0 || app_rows == 1 || app_rows * N == M, "nerf_param_grads: app_rows=%lld", (long long)app_rows);
  TREQUIRE(param_grads_out && packed && workspace && (M == 0 || (save && grad)) && (app_rows == 0 || app),
           "nerf_param_grads: null pointer");
  for (int i = 0; i < P_COUNT; ++i) TREQUIRE(param_grads_out[i], "nerf_param_grads: gradient %d is null", i);
  if (M == 0) return NERF_OK;
  return param_grads(save, grad, M, N, app, app_rows, packed, param_grads_out, dapp, (float*)workspace, ws_bytes / 4,
                     (hipStream_t)stream);
}

size_t nerf_param_grads_workspace_bytes(int64_t M) { return M < 0 ? 0 : max_wgrad_floats(M) * 4; }

int nerf_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
              double beta2, double eps, int64_t step, nerf_stream_t stream) {
  TREQUIRE(n >= 0 && step >= 1, "nerf_adam: n=%lld step=%lld", (long long)n, (long long)step);
  TREQUIRE(n == 0 || (param && grad && exp_avg && exp_avg_sq), "nerf_adam: null pointer");
  return launch_adam(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, (hipStream_t)stream);
}

size_t nerf_train_workspace_bytes(int64_t B, int N) {
  if (B < 0 || N < 1) return 0;
  size_t off[T_COUNT];
  return train_carve(B, N, off);
}

int nerf_train_forward(const float* packed, const float* rays_o, const float* rays_d, int64_t B, double near,
                       double far, int N, const float* t_vals, int perturb, const float* t_rand, uint64_t seed,
                       const float* app, int64_t app_rows, float* rgb_map, float* depth_map, float* weights_out,
                       float* z_out, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  TREQUIRE(B >= 0, "nerf_train_forward: B=%lld", (long long)B);
  if (N < 1 || N > 4096) return set_error(NERF_ERR_UNSUPPORTED, "nerf_train_forward: N=%d (1..4096)", N);
  TREQUIRE(app_rows == 0 || app_rows == 1 || app_rows == B, "nerf_train_forward: app_rows=%lld with B=%lld",
           (long long)app_rows, (long long)B);
  if (B == 0) return NERF_OK;
  TREQUIRE((int64_t)B * N < ((int64_t)1 << 31), "nerf_train_forward: B*N=%lld too large", (long long)B * N);
  TREQUIRE(packed && rays_o && rays_d && t_vals && rgb_map && depth_map && workspace && (app_rows == 0 || app),
           "nerf_train_forward: null pointer");
  size_t off[T_COUNT];
  const size_t need = train_carve(B, N, off);
  if (ws_bytes < need) return set_error(NERF_ERR_WORKSPACE, "nerf_train_forward: workspace %zu < %zu bytes", ws_bytes, need);
  char* ws = (char*)workspace;
  auto R = [&](int i) { return (float*)(ws + off[i]); };
  hipStream_t s = (hipStream_t)stream;
  int rc;
  // the directions normalised (render.py:19) by the ray-feature kernel, which writes them to T_DIRS
  if ((rc = launch_ray_features(packed, rays_d, B, app, app_rows, R(T_FEAT), s, R(T_ENCD), R(T_DIRS)))) return rc;
  if ((rc = launch_stratified(rays_o, R(T_DIRS), B, (float)near, (float)(far - near), N, t_vals, perturb, t_rand,
                              seed, R(T_Z), nullptr, s)))
    return rc;                                                                                          // :22
  if ((rc = launch_mlp(packed, rays_o, R(T_DIRS), R(T_Z), B, N, R(T_FEAT), R(T_RGB), R(T_SIG), nullptr, 0, s,
                       R(T_SAVE), R(T_ENCD), (uint32_t*)R(T_MASK))))
    return rc;                                                                                          // :49
  remember_forward_arith(workspace, g_mlp_arith);
  if ((rc = launch_composite(R(T_RGB), R(T_SIG), R(T_Z), B, N, rgb_map, depth_map, weights_out, s))) return rc;  // :56-80
  if (z_out && hipMemcpyAsync(z_out, R(T_Z), (size_t)B * N * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "nerf_train_forward: z copy failed");
  return NERF_OK;
}

int nerf_train_backward(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                        int64_t B, int N, const float* app, int64_t app_rows, float* const* param_grads_out,
                        float* dapp, float* loss, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  TREQUIRE(B >= 0 && N >= 1 && N <= 4096, "nerf_train_backward: B=%lld N=%d", (long long)B, N);
  TREQUIRE(app_rows == 0 || app_rows == 1 || app_rows == B, "nerf_train_backward: app_rows=%lld", (long long)app_rows);
  TREQUIRE(packed && packedT && param_grads_out && loss && workspace && (B == 0 || (rgb_map && target)) &&
               (app_rows == 0 || app),
           "nerf_train_backward: null pointer");
  for (int i = 0; i < P_COUNT; ++i) TREQUIRE(param_grads_out[i], "nerf_train_backward: gradient %d is null", i);
  if (B == 0) return NERF_OK;
  size_t off[T_COUNT];
  const size_t need = train_carve(B, N, off);
  if (ws_bytes < need) return set_error(NERF_ERR_WORKSPACE, "nerf_train_backward: workspace %zu < %zu bytes", ws_bytes, need);
  char* ws = (char*)workspace;
  auto R = [&](int i) { return (float*)(ws + off[i]); };
  hipStream_t s = (hipStream_t)stream;
  // the mask rows exist only when this workspace's forward ran under f16x3; the backward's kernels
  // follow the arithmetic in force now (an f16x3 backward after an f32 forward reads the ReLU masks
  // from the saved activations instead)
  const int fwd_arith = forward_arith(workspace);
  if (fwd_arith < 0)
    return set_error(NERF_ERR_BAD_ARG, "nerf_train_backward: no nerf_train_forward wrote this workspace");
  const uint32_t* masks = fwd_arith == NERF_ARITH_F16X3 ? (const uint32_t*)R(T_MASK) : nullptr;
  const int64_t M = B * N;
  int rc;
  const float scale = (float)(2.0 / (3.0 * (double)B));                                              // train.py:87
  if ((rc = launch_composite_backward(R(T_RGB), R(T_SIG), R(T_Z), rgb_map, target, nullptr, nullptr, B, N, scale,
                                      R(T_DSIG),
                                      R(T_DRGB), R(T_SQE), s)))
    return rc;
  if ((rc = launch_loss(R(T_SQE), B, loss, s))) return rc;
  if ((rc = launch_mlp_backward(packed, packedT, R(T_SAVE), masks, R(T_SIG), R(T_RGB), R(T_DSIG), R(T_DRGB), M,
                                R(T_GRAD), s, /*store_dhd=*/!fused_ray_sums(N))))
    return rc;
  const size_t wg_floats = (need - off[T_WG]) / 4;
  return param_grads(R(T_SAVE), R(T_GRAD), M, N, app, app_rows, packed, param_grads_out, dapp, R(T_WG), wg_floats, s);
}

// ------------------------------------------------------- the training step with an occupancy grid
// (include/nerfmi_train.h "training with an occupancy grid").  Three calls, because the
// library never synchronises and the live count has to reach the host once: sample (normalise, draw
// z, classify into the ascending live list; dead rows of sigma / rgb zero-filled), forward (ray
// features, the gathered forward writing COMPACT save / mask rows, the dense composite) and backward
// (dense composite backward + loss, gather of dsigma / drgb, the per-row MLP backward and weight
// gradients over M_live rows: the N = 1 route of param_grads, enc_d in every save row).
//
// Workspace: train_carve(B, N) (save / masks / grad hold the M_live <= B N compact rows; rgb, sigma,
// dsigma, drgb stay dense), then, each 256-B aligned: the live list (B N int32), the classify block
// counts, and the compact sigma (M), rgb (3M), dsigma (M), drgb (3M).  The count lives in the
// caller's live_count.
enum { TO_LIVE, TO_BLOCKS, TO_SIG, TO_RGB, TO_DSIG, TO_DRGB, TO_COUNT };
static size_t train_occ_carve(int64_t B, int N, size_t* off, size_t* off_occ) {
  size_t at = train_carve(B, N, off);
  const size_t M = (size_t)B * (size_t)N;
  const size_t sizes[TO_COUNT] = {M * 4, occ_block_count_bytes((int64_t)M), M * 4, M * 12, M * 4, M * 12};
  for (int i = 0; i < TO_COUNT; ++i) {
    off_occ[i] = at;
    at += align256(sizes[i]);
  }
  return at;
}
constexpr int64_t kOccMaxSamples = (int64_t)1 << 30;   // the live list's int32 indices (occupancy.hip)
constexpr int kFwdOcc = -2;                            // forward_arith of a workspace an occ forward wrote
// M_live of the last nerf_train_occ_forward on a workspace (host-side, as g_ws_arith)
static std::unordered_map<const void*, int64_t> g_ws_occ_live;
static void remember_occ_forward(const void* ws, int64_t M_live) {
  remember_forward_arith(ws, kFwdOcc);      // nerf_train_backward refuses this workspace (< 0)
  std::lock_guard<std::mutex> lk(g_ws_mu);
  if (g_ws_occ_live.size() > 4096) g_ws_occ_live.clear();
  g_ws_occ_live[ws] = M_live;
}
static int64_t occ_forward_live(const void* ws) {
  if (forward_arith(ws) != kFwdOcc) return -1;
  std::lock_guard<std::mutex> lk(g_ws_mu);
  const auto it = g_ws_occ_live.find(ws);
  return it == g_ws_occ_live.end() ? -1 : it->second;
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

#define TREQUIRE_SHAPE(fn, B, N)                                                                              \
  do {                                                                                                        \
    TREQUIRE((B) >= 0, fn ": B=%lld", (long long)(B));                                                        \
    if ((N) < 1 || (N) > 4096) return set_error(NERF_ERR_UNSUPPORTED, fn ": N=%d (1..4096)", (N));            \
    if ((int64_t)(B) * (N) > kOccMaxSamples)                                                                  \
      return set_error(NERF_ERR_UNSUPPORTED, fn ": %lld samples exceed the limit %lld", (long long)(B) * (N), \
                       (long long)kOccMaxSamples);                                                            \
  } while (0)

size_t nerf_train_occ_workspace_bytes(int64_t B, int N) {
  if (B < 0 || N < 1 || N > 4096 || B * (int64_t)N > kOccMaxSamples) return 0;
  size_t off[T_COUNT], off_occ[TO_COUNT];
  return train_occ_carve(B, N, off, off_occ);
}

int nerf_train_occ_sample(const float* rays_o, const float* rays_d, int64_t B, double near, double far, int N,
                          const float* t_vals, int perturb, const float* t_rand, uint64_t seed, const uint32_t* bits,
                          int G, const float* lo, const float* inv, int32_t* live_count, void* workspace,
                          size_t ws_bytes, nerf_stream_t stream) {
  TREQUIRE_SHAPE("nerf_train_occ_sample", B, N);
  TREQUIRE(bits && lo && inv && live_count, "nerf_train_occ_sample: null pointer");
  TREQUIRE(B == 0 || (rays_o && rays_d && t_vals && workspace), "nerf_train_occ_sample: null pointer");
  if (G < 1 || G > 1024) return set_error(NERF_ERR_UNSUPPORTED, "nerf_train_occ_sample: G=%d outside 1..1024", G);
  size_t off[T_COUNT], off_occ[TO_COUNT];
  const size_t need = train_occ_carve(B, N, off, off_occ);
  if (B > 0 && ws_bytes < need)
    return set_error(NERF_ERR_WORKSPACE, "nerf_train_occ_sample: workspace %zu < %zu bytes", ws_bytes, need);
  char* ws = (char*)workspace;
  auto R = [&](int i) { return (float*)(ws + off[i]); };
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = launch_normalize(rays_d, B, R(T_DIRS), s))) return rc;                                       // render.py:19
  if ((rc = launch_stratified(rays_o, R(T_DIRS), B, (float)near, (float)(far - near), N, t_vals, perturb, t_rand,
                              seed, R(T_Z), nullptr, s)))
    return rc;
  return launch_occ_classify(rays_o, R(T_DIRS), R(T_Z), B, N, bits, G, lo, inv, (int*)(ws + off_occ[TO_LIVE]),
                             live_count, nullptr, R(T_SIG), R(T_RGB), (uint32_t*)(ws + off_occ[TO_BLOCKS]), s);
}

int nerf_train_occ_forward(const float* packed, const float* rays_o, int64_t B, int N, int64_t M_live,
                           const float* app, int64_t app_rows, float* rgb_map, float* depth_map, float* weights_out,
                           float* z_out, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  TREQUIRE_SHAPE("nerf_train_occ_forward", B, N);
  TREQUIRE(M_live >= 0 && M_live <= B * (int64_t)N, "nerf_train_occ_forward: M_live=%lld with B*N=%lld",
           (long long)M_live, (long long)(B * (int64_t)N));
  TREQUIRE(app_rows >= 0, "nerf_train_occ_forward: app_rows=%lld", (long long)app_rows);
  if (app_rows > 1)
    return set_error(NERF_ERR_UNSUPPORTED, "nerf_train_occ_forward: app_rows=%lld (0 or 1: no per-ray appearance rows)",
                     (long long)app_rows);
  if (g_mlp_arith != NERF_ARITH_F16X3)
    return set_error(NERF_ERR_UNSUPPORTED, "nerf_train_occ_forward: the gathered training forward is f16x3 only");
  if (B == 0) return NERF_OK;
  TREQUIRE(packed && rays_o && rgb_map && depth_map && workspace && (app_rows == 0 || app),
           "nerf_train_occ_forward: null pointer");
  size_t off[T_COUNT], off_occ[TO_COUNT];
  const size_t need = train_occ_carve(B, N, off, off_occ);
  if (ws_bytes < need)
    return set_error(NERF_ERR_WORKSPACE, "nerf_train_occ_forward: workspace %zu < %zu bytes", ws_bytes, need);
  char* ws = (char*)workspace;
  auto R = [&](int i) { return (float*)(ws + off[i]); };
  auto RO = [&](int i) { return (float*)(ws + off_occ[i]); };
  hipStream_t s = (hipStream_t)stream;
  int rc;
  // T_DIRS holds the normalised directions (nerf_train_occ_sample): the features from them as they are
  if ((rc = launch_ray_features(packed, R(T_DIRS), B, app, app_rows, R(T_FEAT), s, R(T_ENCD), nullptr))) return rc;
  if ((rc = launch_mlp16_live(packed, rays_o, R(T_DIRS), R(T_Z), N, R(T_FEAT), R(T_ENCD), (const int*)RO(TO_LIVE),
                              M_live, R(T_RGB), R(T_SIG), RO(TO_RGB), RO(TO_SIG), R(T_SAVE), (uint32_t*)R(T_MASK), s)))
    return rc;
  remember_occ_forward(workspace, M_live);
  if ((rc = launch_composite(R(T_RGB), R(T_SIG), R(T_Z), B, N, rgb_map, depth_map, weights_out, s))) return rc;
  if (z_out && hipMemcpyAsync(z_out, R(T_Z), (size_t)B * N * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "nerf_train_occ_forward: z copy failed");
  return NERF_OK;
}

int nerf_train_occ_backward(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                            int64_t B, int N, int64_t M_live, const float* app, int64_t app_rows,
                            float* const* param_grads_out, float* dapp, float* loss, void* workspace, size_t ws_bytes,
                            nerf_stream_t stream) {
  TREQUIRE_SHAPE("nerf_train_occ_backward", B, N);
  TREQUIRE(M_live >= 0 && M_live <= B * (int64_t)N, "nerf_train_occ_backward: M_live=%lld with B*N=%lld",
           (long long)M_live, (long long)(B * (int64_t)N));
  TREQUIRE(app_rows >= 0, "nerf_train_occ_backward: app_rows=%lld", (long long)app_rows);
  if (app_rows > 1)
    return set_error(NERF_ERR_UNSUPPORTED, "nerf_train_occ_backward: app_rows=%lld (0 or 1: no per-ray appearance rows)",
                     (long long)app_rows);
  if (g_mlp_arith != NERF_ARITH_F16X3)
    return set_error(NERF_ERR_UNSUPPORTED, "nerf_train_occ_backward: the gathered training step is f16x3 only");
  TREQUIRE(packed && packedT && param_grads_out && loss && workspace && (B == 0 || (rgb_map && target)) &&
               (app_rows == 0 || app),
           "nerf_train_occ_backward: null pointer");
  for (int i = 0; i < P_COUNT; ++i) TREQUIRE(param_grads_out[i], "nerf_train_occ_backward: gradient %d is null", i);
  if (B == 0) return NERF_OK;
  size_t off[T_COUNT], off_occ[TO_COUNT];
  const size_t need = train_occ_carve(B, N, off, off_occ);
  if (ws_bytes < need)
    return set_error(NERF_ERR_WORKSPACE, "nerf_train_occ_backward: workspace %zu < %zu bytes", ws_bytes, need);
  if (occ_forward_live(workspace) != M_live)
    return set_error(NERF_ERR_BAD_ARG, "nerf_train_occ_backward: no nerf_train_occ_forward with M_live=%lld wrote this "
                     "workspace", (long long)M_live);
  char* ws = (char*)workspace;
  auto R = [&](int i) { return (float*)(ws + off[i]); };
  auto RO = [&](int i) { return (float*)(ws + off_occ[i]); };
  hipStream_t s = (hipStream_t)stream;
  int rc;
  const float scale = (float)(2.0 / (3.0 * (double)B));                                              // train.py:87
  if ((rc = launch_composite_backward(R(T_RGB), R(T_SIG), R(T_Z), rgb_map, target, nullptr, nullptr, B, N, scale,
                                      R(T_DSIG), R(T_DRGB), R(T_SQE), s)))
    return rc;
  if ((rc = launch_loss(R(T_SQE), B, loss, s))) return rc;
  if (M_live == 0) {   // every sample dead: sigma = 0 is a constant of the step, every gradient is zero
    for (int p = 0; p < P_COUNT; ++p)
      if (hipMemsetAsync(param_grads_out[p], 0, param_floats(p) * 4, s) != hipSuccess)
        return set_error(NERF_ERR_HIP, "nerf_train_occ_backward: hipMemsetAsync failed");
    if (dapp && app_rows && hipMemsetAsync(dapp, 0, (size_t)kAppDim * 4, s) != hipSuccess)
      return set_error(NERF_ERR_HIP, "nerf_train_occ_backward: hipMemsetAsync failed");
    return NERF_OK;
  }
  if ((rc = launch_occ_gather_grads(R(T_DSIG), R(T_DRGB), (const int*)RO(TO_LIVE), M_live, RO(TO_DSIG), RO(TO_DRGB),
                                    s)))
    return rc;
  if ((rc = launch_mlp_backward(packed, packedT, R(T_SAVE), (const uint32_t*)R(T_MASK), RO(TO_SIG), RO(TO_RGB),
                                RO(TO_DSIG), RO(TO_DRGB), M_live, R(T_GRAD), s, /*store_dhd=*/true)))
    return rc;
  const size_t wg_floats = (off_occ[0] - off[T_WG]) / 4;
  return param_grads(R(T_SAVE), R(T_GRAD), M_live, 1, app, app_rows, packed, param_grads_out, dapp, R(T_WG),
                     wg_floats, s);
}

int nerf_mlp_forward_train_live(const float* packed, const float* origins, const float* dirs, const float* z_vals,
                                int64_t R, int N, const float* ray_feat, const float* enc_d, const int32_t* live,
                                int64_t M_live, float* rgb, float* sigma, float* rgb_live, float* sigma_live,
                                float* save, uint32_t* masks, nerf_stream_t stream) {
  TREQUIRE_SHAPE("nerf_mlp_forward_train_live", R, N);
  TREQUIRE(M_live >= 0 && M_live <= R * (int64_t)N, "nerf_mlp_forward_train_live: M_live=%lld with R*N=%lld",
           (long long)M_live, (long long)(R * (int64_t)N));
  TREQUIRE(M_live == 0 || (packed && origins && dirs && z_vals && ray_feat && enc_d && live && rgb && sigma &&
                           rgb_live && sigma_live && save && masks),
           "nerf_mlp_forward_train_live: null pointer");
  if (g_mlp_arith != NERF_ARITH_F16X3)
    return set_error(NERF_ERR_UNSUPPORTED, "nerf_mlp_forward_train_live: the gathered kernel is f16x3 only");
  return launch_mlp16_live(packed, origins, dirs, z_vals, N, ray_feat, enc_d, live, M_live, rgb, sigma, rgb_live,
                           sigma_live, save, masks, (hipStream_t)stream);
}

}  // extern "C"
