// Occupancy-grid sample skipping (include/nerfmi.h "occupancy grid"): the kernels that
// classify a launch's samples against a bitfield and compact the live ones into the ascending list
// the gathered render MLP (mlp16s.hip, mlp16s_live_kernel) runs on, and the two that build a grid
// (threshold + pack of a density lattice, 3 x 3 x 3 dilation).
//
// The grid: box lo[3] .. hi[3], G cells per axis, cell (ix, iy, iz) = bit (index & 31) of word
// (index >> 5), index = (iz G + iy) G + ix.  A sample at p = o + d z (the renderer's two roundings)
// is live iff for each axis c, t_c = (p_c - lo_c) * inv_c (one subtraction, one multiplication, each
// rounded: the library is built with -ffp-contract=off) satisfies 0 <= t_c < G (float compares: NaN
// is dead) and the bit of cell ((int)t_x, (int)t_y, (int)t_z) is set.
//
// Compaction is three launches, none of which waits on another workgroup: per-block live counts
// (wave ballot + popcount), a one-block scan of the block counts (which also writes the total), and
// the write pass, which classifies again (three loads and a bit test) rather than keep a mask.  The
// list is ascending: a wave's 32 samples stay on few rays, and the order is reproducible.  Sample
// indices are int32 (a launch spans at most 2^30 samples, capi.hip); every offset that multiplies an
// index by 3 or by n is formed in 64 bits.
#include "common.h"

namespace nerf {

struct OccGridArg {
  const uint32_t* bits;
  int G;
  float lo[3], inv[3];
};

constexpr int kOccBlock = 256;   // samples (threads) per classify block: 4 waves
constexpr int kOccScan = 1024;   // threads of the one-block scan

__device__ __forceinline__ bool occ_live(const OccGridArg& g, const float* __restrict__ o, const float* __restrict__ d,
                                         const float* __restrict__ z, int64_t i, int n) {
  const int64_t r = i / n;
  const float zz = z[i];
  int cell[3];
  bool in = true;
  const float Gf = (float)g.G;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p = o[3 * r + c] + d[3 * r + c] * zz;      // pts (ray_utils.py:86), two roundings
    const float t = (p - g.lo[c]) * g.inv[c];
    in = in && t >= 0.0f && t < Gf;
    cell[c] = in ? (int)t : 0;
  }
  if (!in) return false;
  const uint32_t idx = ((uint32_t)cell[2] * (uint32_t)g.G + (uint32_t)cell[1]) * (uint32_t)g.G + (uint32_t)cell[0];
  return (g.bits[idx >> 5] >> (idx & 31)) & 1u;
}

// pass 1: block_counts[b] = live samples among samples 256 b .. 256 b + 255
__global__ void __launch_bounds__(kOccBlock) occ_count_kernel(OccGridArg g, const float* __restrict__ o,
                                                              const float* __restrict__ d, const float* __restrict__ z,
                                                              int64_t M, int n, uint32_t* __restrict__ block_counts) {
  __shared__ uint32_t wcount[kOccBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kOccBlock + threadIdx.x;
  const bool live = i < M && occ_live(g, o, d, z, i, n);
  const uint64_t b = __ballot(live);
  if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
}

// pass 2 (one block): block_counts -> exclusive prefix sums in place, the total into *live_count.
// Thread t sums a contiguous run of the counts, the 1024 run sums are scanned in LDS, and the run is
// walked again with its offset.
__global__ void __launch_bounds__(kOccScan) occ_scan_kernel(uint32_t* __restrict__ block_counts, int64_t nblocks,
                                                            int* __restrict__ live_count) {
  __shared__ uint32_t part[kOccScan];
  const int64_t per = (nblocks + kOccScan - 1) / kOccScan;
  const int64_t b0 = imin64((int64_t)threadIdx.x * per, nblocks), b1 = imin64(b0 + per, nblocks);
  uint32_t sum = 0;
  for (int64_t b = b0; b < b1; ++b) sum += block_counts[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < kOccScan; off <<= 1) {       // Hillis-Steele, inclusive
    const uint32_t v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t at = part[threadIdx.x] - sum;                // exclusive offset of this thread's run
  for (int64_t b = b0; b < b1; ++b) {
    const uint32_t c = block_counts[b];
    block_counts[b] = at;
    at += c;
  }
  if (threadIdx.x == kOccScan - 1) *live_count = (int)part[kOccScan - 1];
}

// pass 3: the write.  live[offset of the block + live samples before this one in the block] = i;
// optional mask (uint8, 1 = live) and the zero-fill of the dead samples' sigma / rgb rows (a dead row
// must read sigma = 0 and a finite colour: 0 * NaN would poison its ray).
__global__ void __launch_bounds__(kOccBlock) occ_write_kernel(OccGridArg g, const float* __restrict__ o,
                                                              const float* __restrict__ d, const float* __restrict__ z,
                                                              int64_t M, int n,
                                                              const uint32_t* __restrict__ block_offsets,
                                                              int* __restrict__ live, uint8_t* __restrict__ mask,
                                                              float* __restrict__ sigma, float* __restrict__ rgb) {
  __shared__ uint32_t wcount[kOccBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kOccBlock + threadIdx.x;
  const bool live_s = i < M && occ_live(g, o, d, z, i, n);
  const uint64_t b = __ballot(live_s);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) wcount[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  if (i >= M) return;
  if (live_s) {
    uint32_t at = block_offsets[blockIdx.x];
    for (int w = 0; w < wave; ++w) at += wcount[w];
    at += (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    live[at] = (int)i;
  } else {
    if (sigma) sigma[i] = 0.0f;
    if (rgb) {
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[3 * i + c] = 0.0f;
    }
  }
  if (mask) mask[i] = live_s ? 1 : 0;
}

static OccGridArg grid_arg(const uint32_t* bits, int G, const float* lo, const float* inv) {
  OccGridArg g;
  g.bits = bits;
  g.G = G;
  for (int c = 0; c < 3; ++c) {
    g.lo[c] = lo[c];
    g.inv[c] = inv[c];
  }
  return g;
}

size_t occ_block_count_bytes(int64_t M) { return (size_t)((M + kOccBlock - 1) / kOccBlock) * sizeof(uint32_t); }

// M = B n <= 2^30 samples (the callers check).  block_counts: occ_block_count_bytes(M) bytes.
int launch_occ_classify(const float* o, const float* d, const float* z, int64_t B, int n, const uint32_t* bits, int G,
                        const float* lo, const float* inv, int* live, int* live_count, uint8_t* mask,
                        float* sigma_zero, float* rgb_zero, uint32_t* block_counts, hipStream_t s) {
  const int64_t M = B * (int64_t)n;
  if (M == 0) {
    if (hipMemsetAsync(live_count, 0, sizeof(int), s) != hipSuccess)
      return set_error(NERF_ERR_HIP, "occupancy classify: hipMemsetAsync failed");
    return NERF_OK;
  }
  const OccGridArg g = grid_arg(bits, G, lo, inv);
  const int64_t blocks = (M + kOccBlock - 1) / kOccBlock;
  hipLaunchKernelGGL(occ_count_kernel, dim3((unsigned)blocks), dim3(kOccBlock), 0, s, g, o, d, z, M, n, block_counts);
  if (int rc = check_launch("occ_count_kernel")) return rc;
  hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(kOccScan), 0, s, block_counts, blocks, live_count);
  if (int rc = check_launch("occ_scan_kernel")) return rc;
  hipLaunchKernelGGL(occ_write_kernel, dim3((unsigned)blocks), dim3(kOccBlock), 0, s, g, o, d, z, M, n, block_counts,
                     live, mask, sigma_zero, rgb_zero);
  return check_launch("occ_write_kernel");
}

// Training with a grid (train_api.hip, nerf_train_occ_backward): the composite backward runs dense on
// (B, N); the rows of its dsigma / drgb that the live list names are gathered into the compact rows
// the MLP backward reads.  What it formed at dead rows is dropped (sigma = 0 there is a constant).
__global__ void __launch_bounds__(256) occ_gather_grads_kernel(const float* __restrict__ dsigma,
                                                               const float* __restrict__ drgb,
                                                               const int* __restrict__ live, int64_t M_live,
                                                               float* __restrict__ dsigma_live,
                                                               float* __restrict__ drgb_live) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M_live) return;
  const int64_t s = live[i];
  dsigma_live[i] = dsigma[s];
#pragma unroll
  for (int c = 0; c < 3; ++c) drgb_live[3 * i + c] = drgb[3 * s + c];
}

int launch_occ_gather_grads(const float* dsigma, const float* drgb, const int* live, int64_t M_live,
                            float* dsigma_live, float* drgb_live, hipStream_t s) {
  if (M_live == 0) return NERF_OK;
  hipLaunchKernelGGL(occ_gather_grads_kernel, dim3((unsigned)((M_live + 255) / 256)), dim3(256), 0, s, dsigma, drgb,
                     live, M_live, dsigma_live, drgb_live);
  return check_launch("occ_gather_grads_kernel");
}

// ------------------------------------------------------------------------- grid construction
// bit of cell (ix, iy, iz) = any of its s^3 probes of the (sG)^3 lattice (index (z sG + y) sG + x)
// is > threshold (the max over the probes, NaN probes ignored as fmaxf does).  A wave's ballot is two
// words; lanes 0 and 32 store them.
__device__ __forceinline__ void occ_store_ballot(bool bit, int64_t cell, int64_t words, uint32_t* __restrict__ out) {
  const uint64_t b = __ballot(bit);
  const int lane = threadIdx.x & 63;
  const int64_t w = (cell >> 6) * 2 + (lane >> 5);        // (cell - lane is a multiple of 64)
  if ((lane & 31) == 0 && w < words) out[w] = (uint32_t)(lane ? b >> 32 : b);
}

__global__ void __launch_bounds__(256) occ_pack_kernel(const float* __restrict__ lattice, int G, int sp, float thr,
                                                       int64_t cells, int64_t words, uint32_t* __restrict__ bits) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bit = false;
  if (cell < cells) {
    const int ix = (int)(cell % G), iy = (int)((cell / G) % G), iz = (int)(cell / ((int64_t)G * G));
    const int64_t L = (int64_t)sp * G;
    for (int a = 0; a < sp; ++a)
      for (int b = 0; b < sp; ++b)
        for (int c = 0; c < sp; ++c) {
          const int64_t at = (((int64_t)iz * sp + a) * L + ((int64_t)iy * sp + b)) * L + ((int64_t)ix * sp + c);
          bit = bit || lattice[at] > thr;
        }
  }
  occ_store_ballot(bit, cell, words, bits);
}

// 3 x 3 x 3 binary dilation, clamped at the box faces (a neighbour outside the box is unset).
__global__ void __launch_bounds__(256) occ_dilate_kernel(const uint32_t* __restrict__ in, int G, int64_t cells,
                                                         int64_t words, uint32_t* __restrict__ out) {
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool bit = false;
  if (cell < cells) {
    const int ix = (int)(cell % G), iy = (int)((cell / G) % G), iz = (int)(cell / ((int64_t)G * G));
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int x = ix + dx, y = iy + dy, zc = iz + dz;
          if (x < 0 || x >= G || y < 0 || y >= G || zc < 0 || zc >= G) continue;
          const uint32_t idx = ((uint32_t)zc * (uint32_t)G + (uint32_t)y) * (uint32_t)G + (uint32_t)x;
          bit = bit || ((in[idx >> 5] >> (idx & 31)) & 1u);
        }
  }
  occ_store_ballot(bit, cell, words, out);
}

int launch_occ_pack(const float* lattice, int G, int sp, float thr, uint32_t* bits, hipStream_t s) {
  const int64_t cells = (int64_t)G * G * G, words = (cells + 31) / 32;
  hipLaunchKernelGGL(occ_pack_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, lattice, G, sp, thr,
                     cells, words, bits);
  return check_launch("occ_pack_kernel");
}

int launch_occ_dilate(const uint32_t* in, int G, uint32_t* out, hipStream_t s) {
  const int64_t cells = (int64_t)G * G * G, words = (cells + 31) / 32;
  hipLaunchKernelGGL(occ_dilate_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, in, G, cells, words,
                     out);
  return check_launch("occ_dilate_kernel");
}

}  // namespace nerf
