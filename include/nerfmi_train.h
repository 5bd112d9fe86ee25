/*
 * nerfmi_train.h — training entry points of libnerfmi.so (gfx950).
 *
 * They replace the autograd backward and optimizer step of the reference's training loop,
 * src/train.py:13-207: volume_render(perturb=True) → F.mse_loss(rgb, target) (:87) →
 * loss.backward() (:90) → torch.optim.Adam.step() (:91).  Conventions are those of
 * nerfmi.h (device pointers, caller-owned memory, stream-ordered, status codes).
 *
 * Two levels:
 *  - whole step: nerf_train_forward + nerf_train_backward share one workspace
 *    (nerf_train_workspace_bytes) that carries the saved activations between them;
 *  - stages (for tests and other hosts): forward with saves, composite backward, MLP
 *    backward, parameter gradients, generic weight-gradient GEMM, Adam.
 *
 * `params` / `param_grads` arrays are the 24 state_dict tensors in nerf_pack_weights order:
 * pts_linears.{0..7}.{weight,bias}, density_head, dir_linear, appearance_projection,
 * rgb_linear (.weight, .bias each).
 */
#ifndef NERFMI_TRAIN_H
#define NERFMI_TRAIN_H

#include "nerfmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-sample rows the forward saves / the backward writes (floats). */
#define NERF_SAVE_ROW 2400 /* [h0..h3 | enc_x(64) | h4..h7 | enc_d(32) | r_dir(128) | hd(128)] */
#define NERF_GRAD_ROW 2320 /* [dpre_0..7 (256 each) | dpre_dir(128) | dsigma+pad(8) | dhd(128) | drgb(3)+pad(8)] */
/* Both are stored tile-major: per block of 32 samples, feature groups of 8 outermost.  Element f
 * of sample m's row (row length R) is float (m/32)*32*R + (f/8)*256 + (m%32)*8 + f%8, and a buffer
 * of M samples holds NERF_TILE_ROWS(M) rows (the last block whole; its rows past M are zero). */
#define NERF_TILE_ROWS(M) ((((M) + 31) / 32) * 32)
/* Block exponents (ABI 11, f16x3 only): sample j of each 32-sample block carries, in enc_x's pad
 * slot (save feature 1087) the exponent record of h_j (j < 8) or enc_x (j = 8), and in the float after
 * dsigma (gradient feature 2177) that of dpre_{j+1} (j < 7), [dpre_dir | dsigma] (j = 7) or dpre_0
 * (j = 8): -(1000 + e)
 * with e = frexp's exponent of the block's largest |value| (-126 for an all-zero block); 0 = absent.
 * nerf_param_grads' split-f16 weight gradient scales each chunk from them (csrc/layout.h). */
/* ReLU masks the f16x3 training forward writes for the backward (uint32 words per sample):
 * trunk layers 0..7 (256 bits each) and r_dir (128 bits), 272 bytes (csrc/layout.h kMaskRow). */
#define NERF_MASK_ROW 68

/* ---------------------------------------------------------------- whole step
 * Forward of train.py:77-84 (coarse volume_render, n_importance ignored as in
 * render.py:83-86) keeping every activation the backward needs in `workspace`.
 * Arguments as nerf_render_rays with Nf = 0 and ray0 = 0; weights_out (B,N) and z_out (B,N)
 * are nullable (volume_render's extras).  B*N < 2^31. */
size_t nerf_train_workspace_bytes(int64_t B, int N);
int nerf_train_forward(const float* packed, const float* rays_o, const float* rays_d, int64_t B,
                       double near, double far, int N, const float* t_vals, int perturb,
                       const float* t_rand, uint64_t seed, const float* app, int64_t app_rows,
                       float* rgb_map, float* depth_map, float* weights_out, float* z_out,
                       void* workspace, size_t ws_bytes, nerf_stream_t stream);
/* loss = mse(rgb_map, target) (train.py:87) into *loss (device float) and its gradient
 * with respect to every parameter (written, not accumulated) and, when dapp is non-null,
 * to the appearance rows (app_rows x 32).  packedT from nerf_pack_weights_transposed.  The
 * workspace must hold a nerf_train_forward's saves; the mask source follows the arithmetic that
 * forward ran under (NERF_ERR_BAD_ARG if no forward wrote it). */
int nerf_train_backward(const float* packed, const float* packedT, const float* rgb_map,
                        const float* target, int64_t B, int N, const float* app, int64_t app_rows,
                        float* const* param_grads, float* dapp, float* loss, void* workspace,
                        size_t ws_bytes, nerf_stream_t stream);

/* ------------------------------------------------ training with an occupancy grid
 * The whole step on the samples an occupancy grid marks live (nerfmi.h "occupancy grid": the same
 * float rule decides liveness).  A dead sample has sigma = 0 and rgb = 0 before compositing, as a
 * constant of the step: its weight is exactly 0, it multiplies the transmittance by 1 + 1e-10 like
 * any sigma = 0 sample, the MLP is not run on it and no gradient flows through it.  z_out is that of
 * nerf_train_forward for the same seed.  f16x3 only (NERF_ERR_UNSUPPORTED under NERF_ARITH_F32);
 * app_rows is 0 or 1 (per-ray appearance rows: NERF_ERR_UNSUPPORTED); B*N <= 2^30.
 *
 * Three calls, because the library never synchronises and the live count must reach the host once:
 *   nerf_train_occ_sample    normalises the directions, draws the stratified z (the draws of
 *                            nerf_train_forward for the same seed) and classifies: the ascending live
 *                            list in the workspace, its length in *live_count (device int32).  Needs
 *                            no weights.
 *   (the caller copies *live_count to the host and waits for it)
 *   nerf_train_occ_forward   ray features, the gathered forward, the dense composite.
 *                            PRECONDITION: M_live == *live_count of the sample call on this workspace.
 *   nerf_train_occ_backward  loss and gradients as nerf_train_backward; M_live as in the forward
 *                            (NERF_ERR_BAD_ARG if no such forward wrote the workspace).  With
 *                            M_live = 0 every gradient (and dapp) is written as zeros and the loss is
 *                            that of the all-zero rgb_map.
 * The workspace (nerf_train_occ_workspace_bytes, sized for every sample live; 0 for bad shapes) is
 * nerf_train_forward's plus the live list, the classify block counts and the compact sigma, rgb,
 * dsigma, drgb rows; save, mask and gradient rows hold M_live compact rows in the per-row layout
 * (enc_d in every save row, as N < 32). */
size_t nerf_train_occ_workspace_bytes(int64_t B, int N);
int nerf_train_occ_sample(const float* rays_o, const float* rays_d, int64_t B, double near, double far, int N,
                          const float* t_vals, int perturb, const float* t_rand, uint64_t seed,
                          const uint32_t* bits, int G, const float* lo, const float* inv, int32_t* live_count,
                          void* workspace, size_t ws_bytes, nerf_stream_t stream);
int nerf_train_occ_forward(const float* packed, const float* rays_o, int64_t B, int N, int64_t M_live,
                           const float* app, int64_t app_rows, float* rgb_map, float* depth_map,
                           float* weights_out, float* z_out, void* workspace, size_t ws_bytes,
                           nerf_stream_t stream);
int nerf_train_occ_backward(const float* packed, const float* packedT, const float* rgb_map, const float* target,
                            int64_t B, int N, int64_t M_live, const float* app, int64_t app_rows,
                            float* const* param_grads, float* dapp, float* loss, void* workspace, size_t ws_bytes,
                            nerf_stream_t stream);

/* ------------------------------------------------ training with the hierarchical fine pass
 * One step on B rays with a coarse + fine loss, one network for both passes as in the H1 render
 * (nerfmi.h, nerf_render_rays with Nf > 0).
 *
 * Forward: the coarse pass exactly as nerf_train_forward on (B, N) (same draws for the same seed) into
 * coarse_rgb (B,3), coarse_depth (B) and the nullable coarse_weights_out (B,N); the H1 resample of the
 * coarse weights (draws as nerf_render_rays at ray0 = 0, or u_rand (B,Nf); u_lin as there); the forward
 * with saves on the Nf new samples only; the merged composite over N + Nf into rgb_map, depth_map and
 * the nullable weights_out / z_out (B,N+Nf).  The resampled positions are constants of the step: no
 * gradient reaches the coarse weights through them.
 *
 * Backward: loss = mse(rgb_map, target) + coarse_weight * mse(coarse_rgb, target), coarse_weight >= 0.
 * loss[0] (device float) receives the fine mean squared error, loss[1] the coarse one.  A coarse
 * sample's (dsigma, drgb) is the sum of its coarse-composite and merged-composite terms (so coarse rows
 * carry a gradient at coarse_weight = 0 too), a fine sample's its merged term.  The data and weight
 * gradients run once per part ((B*N, N) and (B*Nf, Nf)) and the two parts are added, one float add per
 * element in a fixed order: param_grads and dapp are written, not accumulated, and deterministic.
 *
 * N in 2..256 and Nf in 1..1024 (else NERF_ERR_UNSUPPORTED); B*N and B*Nf < 2^31; app_rows 0, 1 or B;
 * both arithmetics.  Not combined with an occupancy grid.  The workspace (0 bytes for refused shapes)
 * holds both parts' saves; a backward refuses (NERF_ERR_BAD_ARG) a workspace whose last forward was
 * not the hierarchical one, and the dense and occupancy backwards refuse one it wrote. */
size_t nerf_train_hier_workspace_bytes(int64_t B, int N, int Nf);
int nerf_train_hier_forward(const float* packed, const float* rays_o, const float* rays_d, int64_t B,
                            double near, double far, int N, int Nf, const float* t_vals,
                            const float* u_lin, int perturb, const float* t_rand, const float* u_rand,
                            uint64_t seed, const float* app, int64_t app_rows, float* rgb_map,
                            float* depth_map, float* weights_out, float* z_out, float* coarse_rgb,
                            float* coarse_depth, float* coarse_weights_out, void* workspace,
                            size_t ws_bytes, nerf_stream_t stream);
int nerf_train_hier_backward(const float* packed, const float* packedT, const float* rgb_map,
                             const float* coarse_rgb, const float* target, int64_t B, int N, int Nf,
                             double coarse_weight, const float* app, int64_t app_rows,
                             float* const* param_grads, float* dapp, float* loss /* 2 floats */,
                             void* workspace, size_t ws_bytes, nerf_stream_t stream);

/* ------------------------------------------------------- training with a background
 * The three backwards above with the dataset's alpha channel, a background colour and an opacity
 * term (not reference features; additions to ABI 11).  THE FORWARDS ARE UNCHANGED: a
 * _bg backward follows the same forward on the same workspace, takes the rgb_map (and coarse_rgb)
 * that forward returned, and recomputes each ray's opacity acc = (float) sum w (nerfmi.h, "opacity
 * map and background") from the rgb / sigma / z rows the forward left in the workspace: the dense
 * rows, under a grid the dense zero-filled rows, and for the fine pass the merged rows through
 * merged_src.  Per ray, with k = max(0, 1 - acc) and each product and sum rounded on its own:
 *   target' = alpha * target + (1 - alpha) * bg        alpha (B) nullable = 1
 *   final   = rgb_map + k * bg                         bg (bg_rows,3), bg_rows 0 (black), 1 or B
 *   colour loss  = mean over B x 3 of (final - target')^2
 *   opacity loss = mean over B of (acc - alpha)^2
 *   total   = colour + acc_weight * opacity            acc_weight >= 0
 * so d total / d rgb_map = 2 (final - target') / (3B) and d total / d acc = -(bg . that) where k > 0
 * (else 0) + acc_weight * 2 (acc - alpha) / B, which reaches every weight of the ray.  loss receives
 * the parts: dense and grid loss[0] colour, loss[1] opacity; hierarchical four floats, fine colour,
 * coarse colour, fine opacity, coarse opacity, total = fine + coarse_weight * coarse with each part
 * colour + acc_weight * opacity.  rgb_final (B,3) (and coarse_final) nullable: the blended colour.
 * Deterministic (fixed-order reductions, no float atomics).  The scratch lies in the workspace's
 * gradient rows: the workspace sizes above hold.  With every option off (alpha null, bg_rows 0,
 * acc_weight 0) an entry makes its original's calls and returns its bits; the opacity parts then read
 * 0 and rgb_final is rgb_map.  bg_rows outside {0, 1, B}, a null bg with bg_rows > 0 and an acc_weight
 * that is negative or NaN are NERF_ERR_BAD_ARG; every other refusal is the original's. */
int nerf_train_backward_bg(const float* packed, const float* packedT, const float* rgb_map,
                           const float* target, int64_t B, int N, const float* app, int64_t app_rows,
                           float* const* param_grads, float* dapp, float* loss /* 2 floats */,
                           void* workspace, size_t ws_bytes, const float* alpha, const float* bg,
                           int64_t bg_rows, double acc_weight, float* rgb_final, nerf_stream_t stream);
int nerf_train_occ_backward_bg(const float* packed, const float* packedT, const float* rgb_map,
                               const float* target, int64_t B, int N, int64_t M_live, const float* app,
                               int64_t app_rows, float* const* param_grads, float* dapp,
                               float* loss /* 2 floats */, void* workspace, size_t ws_bytes,
                               const float* alpha, const float* bg, int64_t bg_rows, double acc_weight,
                               float* rgb_final, nerf_stream_t stream);
int nerf_train_hier_backward_bg(const float* packed, const float* packedT, const float* rgb_map,
                                const float* coarse_rgb, const float* target, int64_t B, int N, int Nf,
                                double coarse_weight, const float* app, int64_t app_rows,
                                float* const* param_grads, float* dapp, float* loss /* 4 floats */,
                                void* workspace, size_t ws_bytes, const float* alpha, const float* bg,
                                int64_t bg_rows, double acc_weight, float* rgb_final,
                                float* coarse_final, nerf_stream_t stream);

/* ---------------------------------------------------------------- distortion */
/* The distortion loss of the ray weights (mip-NeRF 360), a penalty on the weights alone that is minimal
 * when a ray's weight sits in one short interval.  Per ray of T samples (T = N for
 * the dense and grid steps, N + Nf for a merged set; z non-decreasing), with w_i the forward's float
 * weights alpha_i * (float)T_i and sample i's interval the compositor's, all in double from the float z:
 *   delta_i = (double)z_{i+1} - (double)z_i  (i < T-1),  delta_{T-1} = (double)1e-3f
 *   m_i     = (double)z_i + delta_i / 2                    inv = 1 / (far - near)
 *   l_r         = inv * [ sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i ]
 *   dl_r / dw_k = inv * [ 2 sum_j w_j |m_k - m_j| + (2/3) w_k delta_k ]
 *   distortion loss = mean over the B rays of l_r
 *   total = (colour + acc_weight * opacity) + dist_weight * distortion
 * z carries no gradient.  T = 1: l = 0 and no gradient (the reference's per-sample tensors are empty).  A
 * ray whose weights are all 0 has l = 0 and a gradient of exactly 0.  On a ray whose z descends somewhere
 * the result is finite and otherwise unspecified.
 *
 * nerf_distortion is the stage, on any weights_out / z_out a render or a training forward returned:
 * loss_rays (B) = (float)l_r and g_w (B,T) = (float)(scale * dl_r/dw_k), each nullable, every output
 * rounded once from double; deterministic.  T in 1..4096 (else NERF_ERR_UNSUPPORTED); far <= near or a
 * non-finite bound or scale is NERF_ERR_BAD_ARG.
 *
 * The _dist entries are the _bg entries with the distortion term: their arguments, then dist_weight,
 * near and far in front of the stream.  loss grows by one float per part: dense and grid loss[2] the
 * distortion loss; hierarchical six floats, fine colour, coarse colour, fine opacity, coarse opacity,
 * fine distortion (over the N + Nf merged samples, gradient scale dist_weight / B), coarse distortion
 * (over the N coarse samples, gradient scale coarse_weight * dist_weight / B).  Under a grid the dense
 * zero-filled rows are used: a dead sample has weight 0.  With dist_weight == 0 an entry makes its _bg
 * original's calls and returns its bits, and the distortion floats read 0; with every _bg option off as
 * well the gradient is the plain MSE's plus the distortion term's.  The scratch (the weights, their
 * gradient and the per-ray loss) lies in the workspace's gradient rows: the workspace sizes above hold.
 * dist_weight negative or NaN, and with dist_weight > 0 far <= near or a non-finite bound, are
 * NERF_ERR_BAD_ARG; every other refusal is the original's. */
int nerf_distortion(const float* weights, const float* z_vals, int64_t B, int T, double near, double far,
                    double scale, float* loss_rays, float* g_w, nerf_stream_t stream);
int nerf_train_backward_dist(const float* packed, const float* packedT, const float* rgb_map,
                             const float* target, int64_t B, int N, const float* app, int64_t app_rows,
                             float* const* param_grads, float* dapp, float* loss /* 3 floats */,
                             void* workspace, size_t ws_bytes, const float* alpha, const float* bg,
                             int64_t bg_rows, double acc_weight, float* rgb_final, double dist_weight,
                             double near, double far, nerf_stream_t stream);
int nerf_train_occ_backward_dist(const float* packed, const float* packedT, const float* rgb_map,
                                 const float* target, int64_t B, int N, int64_t M_live, const float* app,
                                 int64_t app_rows, float* const* param_grads, float* dapp,
                                 float* loss /* 3 floats */, void* workspace, size_t ws_bytes,
                                 const float* alpha, const float* bg, int64_t bg_rows, double acc_weight,
                                 float* rgb_final, double dist_weight, double near, double far,
                                 nerf_stream_t stream);
int nerf_train_hier_backward_dist(const float* packed, const float* packedT, const float* rgb_map,
                                  const float* coarse_rgb, const float* target, int64_t B, int N, int Nf,
                                  double coarse_weight, const float* app, int64_t app_rows,
                                  float* const* param_grads, float* dapp, float* loss /* 6 floats */,
                                  void* workspace, size_t ws_bytes, const float* alpha, const float* bg,
                                  int64_t bg_rows, double acc_weight, float* rgb_final,
                                  float* coarse_final, double dist_weight, double near, double far,
                                  nerf_stream_t stream);

/* -------------------------------------------------------------------- stages */
/* nerf_composite_backward_grad_acc and nerf_composite_merged_backward_acc with g_w, a per-sample upstream
 * gradient of the weights themselves ((B,N); merged: (B,N+Nf) in merged order; nullable = 0), added to the
 * sample's d w right after g_acc.  With g_w null the _acc entry's launch and bits. */
int nerf_composite_backward_grad_w(const float* rgb, const float* sigma, const float* z_vals,
                                   const float* grad_rgb_map, const float* grad_depth_map, int64_t B,
                                   int N, float* dsigma, float* drgb, const float* g_acc, float bd,
                                   const float* g_w, nerf_stream_t stream);
int nerf_composite_merged_backward_w(const float* rgb_c, const float* sigma_c, const float* rgb_f,
                                     const float* sigma_f, const uint16_t* merged_src,
                                     const float* z_all, const float* grad_rgb_map,
                                     const float* grad_depth_map, int64_t B, int N, int Nf,
                                     int accumulate_coarse, float* dsigma_c, float* drgb_c,
                                     float* dsigma_f, float* drgb_f, const float* g_acc, float bd,
                                     const float* g_w, nerf_stream_t stream);
/* nerf_composite_backward_grad and nerf_composite_merged_backward with g_acc (B, nullable = 0), the
 * upstream gradient of the ray's opacity acc = sum w (added to every d w of the ray), and bd, the
 * background depth the forward ran with: NaN = the normalised depth, else depth = sum w z + k bd and
 * its term is grad_depth (z_s - bd) where k > 0, grad_depth z_s where k == 0.  The same arithmetic
 * order (double scans, d sigma rounded once); with g_acc null or zero and bd NaN the same bits. */
int nerf_composite_backward_grad_acc(const float* rgb, const float* sigma, const float* z_vals,
                                     const float* grad_rgb_map, const float* grad_depth_map,
                                     int64_t B, int N, float* dsigma, float* drgb, const float* g_acc,
                                     float bd, nerf_stream_t stream);
int nerf_composite_merged_backward_acc(const float* rgb_c, const float* sigma_c, const float* rgb_f,
                                       const float* sigma_f, const uint16_t* merged_src,
                                       const float* z_all, const float* grad_rgb_map,
                                       const float* grad_depth_map, int64_t B, int N, int Nf,
                                       int accumulate_coarse, float* dsigma_c, float* drgb_c,
                                       float* dsigma_f, float* drgb_f, const float* g_acc, float bd,
                                       nerf_stream_t stream);
/* nerf_sample_importance that emits, beside z_all (B,N+Nf), the fine samples alone in sample order
 * (z_fine (B,Nf)) and for each merged slot which sample sits there: merged_src (B,N+Nf) uint16, an
 * index into cat[coarse (N), fine (Nf)].  The form nerf_render_rays uses internally. */
int nerf_sample_importance_src(const float* z_vals, const float* weights, int64_t B, int N, int Nf,
                               const float* u_lin, const float* u_rand, uint64_t seed, float* z_all,
                               float* z_fine, uint16_t* merged_src, nerf_stream_t stream);
/* nerf_composite_backward_grad over the N + Nf merged samples of a ray: merged sample p of ray r is
 * sample e = merged_src[r*(N+Nf) + p] of cat[coarse, fine], row r*N + e of (rgb_c, sigma_c) when e < N,
 * else row r*Nf + e - N of (rgb_f, sigma_f); z from z_all.  Results go to the same split rows (one
 * writer per element); coarse rows take in + term when accumulate_coarse is set, fine rows are always
 * written.  The same arithmetic in the same order as the dense kernel on the gathered rows: the same
 * bits.  N in 1..256, Nf in 1..1024. */
int nerf_composite_merged_backward(const float* rgb_c, const float* sigma_c, const float* rgb_f,
                                   const float* sigma_f, const uint16_t* merged_src, const float* z_all,
                                   const float* grad_rgb_map, const float* grad_depth_map, int64_t B,
                                   int N, int Nf, int accumulate_coarse, float* dsigma_c, float* drgb_c,
                                   float* dsigma_f, float* drgb_f, nerf_stream_t stream);
/* nerf_mlp_forward_train (f16x3 only) on the M_live samples the ascending list `live` names (sample
 * r*N + s of the (R, N) launch): COMPACT row i is sample live[i].  save (NERF_TILE_ROWS(M_live) rows),
 * masks (M_live rows), rgb_live (M_live,3) and sigma_live (M_live) are what nerf_mlp_forward_train at
 * N = 1 writes for the gathered inputs, bit for bit (enc_d in every row, the block exponents of each
 * 32 compact rows, zero padding rows); rgb and sigma (R*N rows) get the listed rows, the others are
 * left untouched.  M_live = 0 launches nothing. */
int nerf_mlp_forward_train_live(const float* packed, const float* origins, const float* dirs,
                                const float* z_vals, int64_t R, int N, const float* ray_feat,
                                const float* enc_d, const int32_t* live, int64_t M_live, float* rgb,
                                float* sigma, float* rgb_live, float* sigma_live, float* save,
                                uint32_t* masks, nerf_stream_t stream);
/* W^T of trunk layers 1..7 and of dir_linear's h-part in MFMA fragment layout. */
size_t nerf_packed_transposed_floats(void);
int nerf_pack_weights_transposed(const float* const* params, float* packedT, nerf_stream_t stream);
int nerf_pack_weights_transposed_host(const float* const* params, float* packedT);

/* nerf_ray_features plus enc_d (R,32): PE_4(d) (models.py:122), zero-padded. */
int nerf_ray_features_train(const float* packed, const float* dirs, int64_t R, const float* app,
                            int64_t app_rows, float* feat, float* enc_d, nerf_stream_t stream);
/* nerf_mlp_forward (no scatter) that also writes save (NERF_TILE_ROWS(R*N), NERF_SAVE_ROW,
 * tile-major, padding rows zeroed; enc_d, constant along a ray, only in each ray's first row when
 * N >= 32) and, under the f16x3
 * arithmetic, masks (R*N, NERF_MASK_ROW) (required there; ignored under f32, may be null). */
int nerf_mlp_forward_train(const float* packed, const float* origins, const float* dirs,
                           const float* z_vals, int64_t R, int N, const float* ray_feat,
                           const float* enc_d, float* rgb, float* sigma, float* save,
                           uint32_t* masks, nerf_stream_t stream);
/* d/d(sigma, rgb) of the composite (render.py:66-78) given g = scale*(rgb_map - target);
 * sq_err (B) = per-ray sum of squared errors. */
int nerf_composite_backward(const float* rgb, const float* sigma, const float* z_vals,
                            const float* rgb_map, const float* target, int64_t B, int N,
                            float scale, float* dsigma, float* drgb, float* sq_err,
                            nerf_stream_t stream);
/* The same for an arbitrary upstream gradient (autograd of volume_render, src/render.py:56-80):
 * grad_rgb_map (B,3) = d loss / d rgb_map, grad_depth_map (B) = d loss / d depth_map, each
 * nullable (= 0); dsigma (B,N), drgb (B,N,3) out. */
int nerf_composite_backward_grad(const float* rgb, const float* sigma, const float* z_vals,
                                 const float* grad_rgb_map, const float* grad_depth_map, int64_t B,
                                 int N, float* dsigma, float* drgb, nerf_stream_t stream);
/* Data gradients of NeRF.forward (models.py:105-162) on MFMA: grad (NERF_TILE_ROWS(M),
 * NERF_GRAD_ROW, tile-major; save as the forward wrote it).  Under
 * f16x3 the ReLU masks come from `masks` when non-null (an f16x3 forward's), else from the saved
 * activations; the f32 backward always reads the activations. */
int nerf_mlp_backward(const float* packed, const float* packedT, const float* save,
                      const uint32_t* masks, const float* sigma, const float* rgb,
                      const float* dsigma, const float* drgb, int64_t M, float* grad,
                      nerf_stream_t stream);
/* Every parameter gradient (+ appearance rows) from the tile-major save and grad rows. */
size_t nerf_param_grads_workspace_bytes(int64_t M);
int nerf_param_grads(const float* save, const float* grad, int64_t M, int N, const float* app,
                     int64_t app_rows, const float* packed, float* const* param_grads, float* dapp,
                     void* workspace, size_t ws_bytes, nerf_stream_t stream);
/* Plain row-major operands: out_w[n][k] = sum_m a[m*lda+n] x[(m/x_div)*ldx+k] (x_div 0: row 0), out_b[n] = sum_m a[m*lda+n]
 * (nullable); accumulate adds to the outputs instead of overwriting. */
size_t nerf_wgrad_workspace_bytes(int64_t M, int N, int K);
int nerf_wgrad(const float* a, int64_t lda, int N, const float* x, int64_t ldx, int K, int64_t x_div,
               int64_t M, float* out_w, float* out_b, int accumulate, void* workspace,
               size_t ws_bytes, nerf_stream_t stream);
/* torch.optim.Adam step (amsgrad off, no weight decay), `step` counted from 1. */
int nerf_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
              double lr, double beta1, double beta2, double eps, int64_t step, nerf_stream_t stream);

/* ------------------------------------------------ position gradient and normals
 * (not reference features; additions to ABI 11)
 *
 * Position gradient.  For a sample with position x (the forward's o + d*z, as rounded there), save row S
 * and gradient row G:
 *   g_enc[f] = sum_n W0[n][f] dpre_0[n] + sum_n W4[n][256+f] dpre_4[n]          f = 0..62
 * with W0 = pts_linears.0.weight (256 x 63) and W4 = pts_linears.4.weight (256 x 319, columns 256..318
 * the skip's encoding part); features in the reference order [x, sin x, cos x, sin 2x, cos 2x, ...] in
 * blocks of 3; and for component c
 *   dx[c] = g_enc[c] + sum_{k=0..9} 2^k ( cos(2^k x_c) g_enc[3+6k+c] - sin(2^k x_c) g_enc[6+6k+c] )
 * The sines and cosines are the saved enc_x values of S (no second trigonometric evaluation; 2^k is an
 * exact scaling).  Slot 63 of enc_x is not data (under f16x3 it holds a block-exponent record) and is
 * never read as a feature.  dx is d loss / d x for whatever (dsigma, drgb) nerf_mlp_backward was given.
 *
 * Density gradient: the same with dsigma = 1, drgb = 0: the gradient of sigma, exactly 0 where
 * sigma = 0 (the chain's density-head mask is sigma > 0).
 * Normal of a sample: n = -g / sqrt(g.g + 1e-30) with g the density gradient; g = 0 gives n = 0.
 * Normal map: normal_map = sum_i w_i n_i over the sample set and weights a render returned (with a fine
 * pass: the merged set and the fine weights).  World space, pointing out of the surface, NOT
 * renormalised: its length is at most the ray's opacity, and a short vector means the weights straddle
 * disagreeing normals.  A dead sample of an occupancy grid has weight exactly 0 and adds nothing. */
/* W0^T and W4[:,256:319]^T as one 64 x 512 MFMA operand (row 63 zero), a buffer of its own
 * (csrc/layout.h "input-gradient weights"). */
size_t nerf_packed_input_floats(void);
int nerf_pack_weights_input(const float* const* params, float* packedIn, nerf_stream_t stream);
int nerf_pack_weights_input_host(const float* const* params, float* packedIn);
/* dx (M,3) from the tile-major save rows of nerf_mlp_forward_train and gradient rows of nerf_mlp_backward
 * (either arithmetic: only the f32 rows are read).  Rows past M store nothing. */
int nerf_mlp_position_grad(const float* packedIn, const float* save, const float* grad, int64_t M,
                           float* dx, nerf_stream_t stream);
/* normal_map (B,3) = sum_i weights[r][i] n(dx[r][i]) over dx (B,T,3) and weights (B,T), in double, each
 * component rounded once, in a fixed order: a ray's result does not depend on the launch's size.
 * T in 1..4096 (else NERF_ERR_UNSUPPORTED). */
int nerf_composite_normals(const float* dx, const float* weights, int64_t B, int T, float* normal_map,
                           nerf_stream_t stream);
/* The normal map of rays a render returned z_vals (B,T) and weights (B,T) for: per chunk of rays (at
 * most 2^18 samples, lowered further by the library's launch limit) nerf_ray_features_train without
 * appearance, nerf_mlp_forward_train on the given z_vals, nerf_mlp_backward with dsigma = 1 and drgb = 0,
 * nerf_mlp_position_grad, nerf_composite_normals.  rays_d_normalised as nerf_normalize_dirs returns them.
 * The workspace holds one chunk (0 bytes for refused shapes).  T in 1..4096. */
size_t nerf_render_normals_workspace_bytes(int64_t B, int T);
int nerf_render_normals(const float* packed, const float* packedT, const float* packedIn,
                        const float* rays_o, const float* rays_d_normalised, const float* z_vals,
                        const float* weights, int64_t B, int T, float* normal_map, void* workspace,
                        size_t ws_bytes, nerf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFMI_TRAIN_H */
