// What decides a weight-gradient launch (wgrad.hip), as pure host functions of the shape: the chunk
// policy, the workspace sizers and wgrad_plan, the route launch_wgrad takes.  No HIP types and no
// globals (layout.h only), so a plain host compiler builds it: tests/wgrad_plan_dump.cpp prints the
// plan over a grid of shapes and tests/test_wgrad_plan.py checks that the sizers bound every route.
#pragma once
#include "layout.h"

namespace nerf {

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

// The partial buffer of a (N, K) weight gradient over M samples: the policy's chunks.  No route of
// wgrad_plan has more (the fp32 routes' kWChunk is the longest chunk): tests/test_wgrad_plan.py.
inline size_t wgrad_workspace_floats(int64_t M, int N, int K) {
  const int clen = wgrad_chunk_len(N, K, M);
  const int64_t chunks = (M + clen - 1) / clen;
  return (size_t)chunks * wgrad_stride(N, K);
}

// the largest wgrad partial buffer over the parameter list of param_grads (one stream's)
inline size_t wgrad_stream_floats(int64_t M) {
  const int Ks[] = {kPosEnc, kHidden, kHidden + kPosEnc, kHidden + kDirEnc, kAppDim, kDirHidden};
  size_t m = 0;
  for (int K : Ks) {
    const size_t f = wgrad_workspace_floats(M, kHidden, K);
    if (f > m) m = f;
  }
  return m;
}

// The rgb head's streaming launch (wgrad_head3_kernel): chunks of kHeadChunkBlocks 32-sample blocks.
constexpr int kHeadChunkBlocks = 16;   // (512 chunks per 262K-sample step: two workgroups per CU)
inline int wgrad_head3_chunks(int64_t M) { return (int)(((M + 31) / 32 + kHeadChunkBlocks - 1) / kHeadChunkBlocks); }
// The layer-0 / skip-PE pair (wgrad_pair16_kernel): the policy's chunks of a 512 x 63 GEMM.
inline int wgrad_pair_clen(int64_t M) { return wgrad_chunk_len(2 * kHidden, kPosEnc, M); }
inline int wgrad_pair_chunks(int64_t M) { return (int)((M + wgrad_pair_clen(M) - 1) / wgrad_pair_clen(M)); }

// One value per kernel family and tile shape that launch_wgrad starts.
enum class WgradRoute {
  Fallback,      // wgrad_kernel: fp32 MFMA on unaligned operands
  Lds128x128,    // wgrad_lds_kernel<2, 2>: fp32 MFMA, LDS-staged
  Lds256x64,     // wgrad_lds_kernel<4, 1>
  Bf128x128,     // wgrad_bf_kernel<2, 2>: bf16x6
  Bf256x64,      // wgrad_bf_kernel<4, 1>
  BfK64,         // wgrad_bf_k64_kernel: bf16x6, 256 x (K <= 64), one x row per sample
  H16Whole,      // wgrad_h16w_kernel: split f16, the 256 x 256 tile in one workgroup (row-major rows)
  H16Half        // wgrad_h16h_kernel: split f16, two half-tile workgroups (tile-major rows)
};

struct WgradPlan {
  WgradRoute route;
  int clen, chunks;      // samples per chunk, chunks of the launch
  bool x_blk;            // x tile-major (tiled, x_tiled and one x row per sample)
  bool xd1;              // one x row per sample, read in a's layout: the stage-invariant x loader
  bool scaled;           // the partials carry chunk exponents (the split-f16 whole-tile kernels)
  bool writes_sums;      // the launch can write d pre_dir's 8-sample sums
  size_t partial_floats; // chunks * wgrad_stride(N, K)
};

constexpr int kWgradArithF16x3 = 1;   // NERF_ARITH_F16X3 (train_internal.h asserts it)

// arith: the MLP arithmetic in force; aligned: a, x 16-byte aligned with row lengths % 4 == 0; tiled /
// x_tiled: a / x tile-major rows (layout.h).  Under the split arithmetic the buffer offsets of a
// chunk's rows must stay below 2^31 (lda, ldx < 2^18): the whole-tile GEMMs on split-f16 MFMA, the
// rest on bf16x6.
inline WgradPlan wgrad_plan(int arith, int N, int K, int64_t x_div, int64_t M, int64_t lda, int64_t ldx, bool aligned,
                            bool tiled, bool x_tiled) {
  WgradPlan p{};
  p.x_blk = tiled && x_tiled && x_div == 1;
  p.xd1 = x_div == 1 && (!tiled || p.x_blk);
  p.clen = kWChunk;
  if (arith == kWgradArithF16x3 && K >= 1 && lda < (1 << 18) && ldx < (1 << 18)) {
    p.clen = wgrad_chunk_len(N, K, M);
    if (wgrad_whole_tile(N, K) && x_div == 1 && tiled && p.x_blk) {
      // tile-major rows (the training path): two workgroups per CU, half the rows each; the
      // dir_linear + density launch (N = 160) keeps 160 of 256 rows
      p.route = WgradRoute::H16Half;
      p.scaled = p.writes_sums = true;
    } else if (N == 256 && wgrad_whole_tile(N, K) && x_div == 1 && !tiled) {   // nerf_wgrad's row-major operands
      p.route = WgradRoute::H16Whole;
      p.scaled = true;
    } else if (N == 256 && K <= 64 && x_div == 1 && (!tiled || p.x_blk)) {
      p.route = WgradRoute::BfK64;
    } else if (K <= 64 && N > 64) {
      p.route = WgradRoute::Bf256x64;
    } else {
      p.route = WgradRoute::Bf128x128;
    }
  } else if (aligned && K >= 1 && K <= 64 && N > 64) {
    p.route = WgradRoute::Lds256x64;
  } else if (aligned && K >= 1) {
    p.route = WgradRoute::Lds128x128;
  } else {
    p.route = WgradRoute::Fallback;
  }
  p.chunks = (int)((M + p.clen - 1) / p.clen);
  p.partial_floats = (size_t)p.chunks * wgrad_stride(N, K);
  return p;
}

}  // namespace nerf
