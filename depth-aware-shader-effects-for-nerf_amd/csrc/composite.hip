// Alpha compositing of volume_render (R7): 16 lanes per ray, 4 consecutive samples per lane.
//
// Reference: src/render.py:56-80.
//   dists = [z[s+1]-z[s], 1e-3]  alpha = 1 - exp(-sigma*dist)
//   T = exclusive cumprod(1 - alpha + 1e-10)   w = alpha*T
//   rgb_map = sum w*c     depth = sum w*z / (sum w + 1e-10)
// torch's CPU cumprod accumulates in double and rounds each prefix to float; the kernel
// computes the same prefixes as a double-precision product scan (below), the running product
// carried across 64-sample rounds.  Sums accumulate the reference's float products in double and
// round once.
//
// N == 1 reproduces the reference's degenerate case: z[1:]-z[:-1] is empty and so is the
// padded dists tensor (render.py:56-58 pads with ones_like of an empty slice), every
// per-sample tensor is empty and both maps are 0.
//
// Bound: HBM.  Reads 20 B/sample (rgb 12, sigma 4, z 4), writes 16 B/ray (+4 B/sample of
// weights when requested).
//
// Layout of the work: 16 lanes (one DPP row) per ray, 4 rays per wave.  A ray is taken in rounds
// of 64 samples; in a round lane k owns samples 4k .. 4k+3 (contiguous: 16-byte loads of z, sigma
// and the 48 bytes of rgb when the buffers allow, one 16-byte store of weights).  Per round: the
// lane's product of its 4 factors, an exclusive product scan over the row's 16 lanes in double
// (4 `row_shr` DPP steps, no LDS), each sample's T = carry * row prefix * lane prefix (products in
// double, rounded once to float), and the lane's running sums.  The row's last lane carries the
// product into the next round; the sums are added over the row by 4 DPP steps at the end.  (One
// wave per ray with 64-lane shuffle scans and reductions through ds_bpermute ran 0.50 / 0.88 ms for
// the 800^2 coarse / fine composite, 0.28 of HBM bandwidth: it was bound by the cross-lane traffic.)
#include "common.h"

namespace nerf {

// v from the lane `off` below in the same 16-lane row; lanes below off get `fill`
template <int OFF>
__device__ __forceinline__ double row_shr(double v, double fill) {
  const long long b = __builtin_bit_cast(long long, v), fb = __builtin_bit_cast(long long, fill);
  const int lo = __builtin_amdgcn_update_dpp((int)fb, (int)b, 0x110 + OFF, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(fb >> 32), (int)(b >> 32), 0x110 + OFF, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
// inclusive product / sum over lanes 0..k of the row
__device__ __forceinline__ double row_scan_mul(double v) {
  v *= row_shr<1>(v, 1.0);
  v *= row_shr<2>(v, 1.0);
  v *= row_shr<4>(v, 1.0);
  v *= row_shr<8>(v, 1.0);
  return v;
}
__device__ __forceinline__ double row_scan_add(double v) {
  v += row_shr<1>(v, 0.0);
  v += row_shr<2>(v, 0.0);
  v += row_shr<4>(v, 0.0);
  v += row_shr<8>(v, 0.0);
  return v;
}

// MERGED (the fine composite of nerf_render_rays): sample s of ray r is sample src[r N + s] of
// cat[coarse, fine] (importance.hip's merged_src), gathered from the coarse pass's and the fine MLP's
// outputs, which both lie in sample order; z comes from the merged z row.  The same values in the
// same order as compositing rows the coarse results were scattered into: the same bits.
struct MergedSrc {
  const float* rgb_c;
  const float* sigma_c;
  const float* rgb_f;
  const float* sigma_f;
  const uint16_t* src;
  int nc, nf;
};

// VEC: every pointer 16-byte aligned and N % 4 == 0, so a lane's 4 samples load as one f32x4.
// STAGE (MERGED, T <= kStageT): 8 rays per block; their coarse and fine (rgb, sigma) are first copied
// into LDS as one (r, g, b, sigma) quad per cat index, with whole-row coalesced loads, and the
// composite gathers from there (gathering each sample's 16 bytes from global memory cost 1.14 ms
// for the 800^2 fine pass against 0.18 ms of staging).
constexpr int kStageT = 256;

// composite_bg_kernel: the ray's opacity acc = (float) sum w, the composite's own
// double sum rounded once, goes to acc_map (nullable), and with k = max(0, 1 - acc)
//   rgb_map += k * bg[r]            (bg null: no blend; stride 0: one colour, 3: one per ray)
//   depth    = (float) sum w z + k * bd   (bd NaN: the normalised depth above)
// each product rounded, then each sum (the library is built without contraction).  An empty ray has
// acc == 0 and k == 1: colour == bg and depth == bd, bit for bit.  (CompositeBg: common.h.)
//
// The kernel, twice (composite_body.h): the plain kernel's text is untouched by the second inclusion.
#define COMPOSITE_BG 0
#include "composite_body.h"
#undef COMPOSITE_BG
#define COMPOSITE_BG 1
#include "composite_body.h"
#undef COMPOSITE_BG

int launch_composite(const float* rgb, const float* sigma, const float* z, int64_t B, int N, float* rgb_map,
                     float* depth, float* weights, hipStream_t s) {
  if (B == 0) return NERF_OK;
  const bool vec = N % 4 == 0 && (uintptr_t)rgb % 16 == 0 && (uintptr_t)sigma % 16 == 0 && (uintptr_t)z % 16 == 0 &&
                   (!weights || (uintptr_t)weights % 16 == 0);
  const dim3 grid((unsigned)((B + 15) / 16));
  const MergedSrc none{};
  if (vec)
    hipLaunchKernelGGL((composite_kernel<true, false>), grid, dim3(256), 0, s, rgb, sigma, z, B, N, rgb_map, depth,
                       weights, none);
  else
    hipLaunchKernelGGL((composite_kernel<false, false>), grid, dim3(256), 0, s, rgb, sigma, z, B, N, rgb_map, depth,
                       weights, none);
  return check_launch("composite_kernel");
}

int launch_composite_merged(const float* rgb_c, const float* sigma_c, const float* rgb_f, const float* sigma_f,
                            const uint16_t* src, const float* z_all, int64_t B, int N, int Nf, float* rgb_map,
                            float* depth, float* weights, hipStream_t s) {
  if (B == 0) return NERF_OK;
  const int T = N + Nf;
  const bool vec = T % 4 == 0 && (uintptr_t)z_all % 16 == 0 && (!weights || (uintptr_t)weights % 16 == 0);
  const dim3 grid((unsigned)((B + 15) / 16));
  const MergedSrc ms{rgb_c, sigma_c, rgb_f, sigma_f, src, N, Nf};
  if (T <= kStageT) {
    const size_t lds = (size_t)8 * T * sizeof(f32x4);
    const dim3 grid8((unsigned)((B + 7) / 8));
    if (vec)
      hipLaunchKernelGGL((composite_kernel<true, true, true>), grid8, dim3(128), lds, s, nullptr, nullptr, z_all, B, T,
                         rgb_map, depth, weights, ms);
    else
      hipLaunchKernelGGL((composite_kernel<false, true, true>), grid8, dim3(128), lds, s, nullptr, nullptr, z_all, B, T,
                         rgb_map, depth, weights, ms);
  } else if (vec)
    hipLaunchKernelGGL((composite_kernel<true, true>), grid, dim3(256), 0, s, nullptr, nullptr, z_all, B, T, rgb_map,
                       depth, weights, ms);
  else
    hipLaunchKernelGGL((composite_kernel<false, true>), grid, dim3(256), 0, s, nullptr, nullptr, z_all, B, T, rgb_map,
                       depth, weights, ms);
  return check_launch("composite_kernel (merged)");
}

// The same grids, blocks and LDS with composite_bg_kernel (the merged form stages whole rows as above).
int launch_composite_bg(const float* rgb, const float* sigma, const float* z, int64_t B, int N, float* rgb_map,
                        float* depth, float* weights, const CompositeBg& bga, hipStream_t s) {
  if (B == 0) return NERF_OK;
  const bool vec = N % 4 == 0 && (uintptr_t)rgb % 16 == 0 && (uintptr_t)sigma % 16 == 0 && (uintptr_t)z % 16 == 0 &&
                   (!weights || (uintptr_t)weights % 16 == 0);
  const dim3 grid((unsigned)((B + 15) / 16));
  const MergedSrc none{};
  if (vec)
    hipLaunchKernelGGL((composite_bg_kernel<true, false>), grid, dim3(256), 0, s, rgb, sigma, z, B, N, rgb_map, depth,
                       weights, none, bga);
  else
    hipLaunchKernelGGL((composite_bg_kernel<false, false>), grid, dim3(256), 0, s, rgb, sigma, z, B, N, rgb_map, depth,
                       weights, none, bga);
  return check_launch("composite_bg_kernel");
}

int launch_composite_merged_bg(const float* rgb_c, const float* sigma_c, const float* rgb_f, const float* sigma_f,
                               const uint16_t* src, const float* z_all, int64_t B, int N, int Nf, float* rgb_map,
                               float* depth, float* weights, const CompositeBg& bga, hipStream_t s) {
  if (B == 0) return NERF_OK;
  const int T = N + Nf;
  const bool vec = T % 4 == 0 && (uintptr_t)z_all % 16 == 0 && (!weights || (uintptr_t)weights % 16 == 0);
  const dim3 grid((unsigned)((B + 15) / 16));
  const MergedSrc ms{rgb_c, sigma_c, rgb_f, sigma_f, src, N, Nf};
  if (T <= kStageT) {
    const size_t lds = (size_t)8 * T * sizeof(f32x4);
    const dim3 grid8((unsigned)((B + 7) / 8));
    if (vec)
      hipLaunchKernelGGL((composite_bg_kernel<true, true, true>), grid8, dim3(128), lds, s, nullptr, nullptr, z_all, B,
                         T, rgb_map, depth, weights, ms, bga);
    else
      hipLaunchKernelGGL((composite_bg_kernel<false, true, true>), grid8, dim3(128), lds, s, nullptr, nullptr, z_all, B,
                         T, rgb_map, depth, weights, ms, bga);
  } else if (vec)
    hipLaunchKernelGGL((composite_bg_kernel<true, true>), grid, dim3(256), 0, s, nullptr, nullptr, z_all, B, T, rgb_map,
                       depth, weights, ms, bga);
  else
    hipLaunchKernelGGL((composite_bg_kernel<false, true>), grid, dim3(256), 0, s, nullptr, nullptr, z_all, B, T,
                       rgb_map, depth, weights, ms, bga);
  return check_launch("composite_bg_kernel (merged)");
}

}  // namespace nerf
