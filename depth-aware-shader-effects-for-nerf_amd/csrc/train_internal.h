// What crosses the training translation units (composite_bwd.hip, mlp_backward.hip, wgrad.hip,
// adam.hip, train_api.hip): the launchers' prototypes, the host structs passed between
// them, the weight gradients' chunk policy and workspace sizers, and the f32 MFMA wrapper.  The
// transposed-weight layout is in layout.h; no kernel is defined here.
#pragma once
#include "common.h"

namespace nerf {

static_assert(kSaveRow == NERF_SAVE_ROW && kGradRow == NERF_GRAD_ROW, "nerfmi_train.h rows out of sync");

__device__ __forceinline__ f32x16 mfma32t(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// ------------------------------------------------------- weight gradient: chunks and workspace
constexpr int kWChunk = 2048;   // samples per chunk
// Chunk length of a (N, K) weight gradient outside the split-f16 GEMMs: short enough that a 2^18-sample
// step puts a block in every resident slot.  The 256x64-tile launches (K <= 64, N > 64: layer 0
// and the appearance projection) hold one block per CU and have one tile: 1024-sample chunks give
// 256 blocks instead of 128.  The 128x128-tile launches hold two blocks per CU; those with fewer
// than 3 tiles (the sigma and rgb heads) take 1024 / 512-sample chunks.
// (N = 160: dir_linear's 128 rows + the density head's, the tile-major training path only)
inline bool wgrad_whole_tile(int N, int K) { return (N == 256 || N == 160) && K == 256; }
// Whole-tile chunks of 2,048 samples (128 per 262K-sample step, half the CUs): on split-f16 the
// launches are bound by HBM, not MFMA, and halving the chunk partials (~0.5 GB per step written and
// read back) paid +1.7 % on the training step against 1,024-sample chunks (same-box A/B,
// profiles/r05/ab_head3_pe_clen2k.log; under bf16x6 the 2,048-sample chunks had been 3.5 % slower).
// (Round 6, same box: 4,096-sample whole-tile chunks -11 % on the step, 64 chunks leave CUs idle; the
// layer-0 / skip-PE pair on 2,048-sample chunks instead of 1,024 +1.1 %, its partials halved:
// profiles/r06/ab_train_chunks.log.)
constexpr int kWholeClen = kWChunk, kWholeMinChunks = 128;       // whole-tile chunk length, minimum chunk count
constexpr int kPairClen = kWChunk, kPairMinChunks = 128;          // the layer-0 / skip-PE pair's
inline int wgrad_chunk_len_big(int N, int K) {
  if (wgrad_whole_tile(N, K)) return kWholeClen;   // one block per chunk, 256 per step
  if (K <= 64 && N == 2 * kHidden) return kPairClen;   // (the layer-0 / skip-PE pair)
  if (K <= 64 && N > 64) return kWChunk / 2;       // (wgrad_bf_k64_kernel: 512-sample chunks ran the GEMM
                                                    // 3 % faster but doubled the reduction)
  const int tiles = ((N + 127) / 128) * ((K + 127) / 128);
  return tiles == 1 ? kWChunk / 4 : tiles == 2 ? kWChunk / 2 : kWChunk;
}
// Short GEMMs (the per-ray ones over B rows) halve the chunk down to one 16-sample stage until
// there are >= 256 chunks: 4,096 rays in 1,024-row chunks ran 8 blocks, 80-100 us per launch.
inline int wgrad_chunk_len(int N, int K, int64_t M) {
  int c = wgrad_chunk_len_big(N, K);
  const int min_chunks = wgrad_whole_tile(N, K) ? kWholeMinChunks : (K <= 64 && N == 2 * kHidden) ? kPairMinChunks : 256;
  while (c > 16 && (M + c - 1) / c < min_chunks) c /= 2;
  return c;
}

// (+ 4 trailing floats: the split-f16 kernel's chunk exponent, wgrad_h16w_kernel)
NERF_HD inline int64_t wgrad_stride(int N, int K) { return ((((int64_t)N * (K + 1)) + 3) & ~(int64_t)3) + 4; }

inline size_t wgrad_workspace_floats(int64_t M, int N, int K) {
  const int clen = wgrad_chunk_len(N, K, M);   // >= the chunk count of every path of launch_wgrad
  const int64_t chunks = (M + clen - 1) / clen;
  return (size_t)chunks * wgrad_stride(N, K);
}

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
// composite_bwd.hip
int launch_composite_backward(const float* rgb, const float* sigma, const float* z, const float* rgb_map,
                              const float* target, const float* grad_map, const float* grad_depth, int64_t B, int N,
                              float scale, float* dsigma, float* drgb, float* sq_err, hipStream_t s);
// mlp_backward.hip
int launch_packT(const float* const* params, float* packedT, hipStream_t s);
void packT_host(const float* const* params, float* packedT);
int launch_mlp_backward(const float* packed, const float* packedT, const float* save, const uint32_t* masks,
                        const float* sigma, const float* rgb, const float* dsigma, const float* drgb, int64_t M,
                        float* grad, hipStream_t s, bool store_dhd = true);
// wgrad.hip (the weight gradients)
int launch_wgrad(const float* a, int64_t lda, int N, const float* x, int64_t ldx, int K, int64_t x_div, int64_t M,
                 float* out_w, int ldo, float* out_b, int accumulate, float* ws, hipStream_t s,
                 const WgradSplit* split = nullptr, bool tiled = false, bool x_tiled = true,
                 const H16Meta* meta = nullptr, float* sums = nullptr);
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

}  // namespace nerf
