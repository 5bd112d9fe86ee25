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
#include "composite_plan.h"

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
// for the 800^2 fine pass against 0.18 ms of staging).  Which variant, grid, block and LDS a call takes:
// composite_plan.h (kStageT is there).

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

// One variant, plain or with the background (the same grid, block and LDS).  The merged forms take null
// rgb / sigma and T as the kernel's N.
template <bool VEC, bool MERGED, bool STAGE = false>
static void launch_variant(const CompositePlan& p, const CompositeSamples& in, float* rgb_map, float* depth,
                           float* weights, const CompositeBg* bga, hipStream_t s) {
  const MergedSrc ms = MERGED ? MergedSrc{in.rgb, in.sigma, in.rgb_f, in.sigma_f, in.src, in.N, in.Nf} : MergedSrc{};
  const float* rgb = MERGED ? nullptr : in.rgb;
  const float* sigma = MERGED ? nullptr : in.sigma;
  const int n = in.N + in.Nf;
  if (bga)
    hipLaunchKernelGGL((composite_bg_kernel<VEC, MERGED, STAGE>), dim3(p.grid), dim3(p.block), p.lds, s, rgb, sigma,
                       in.z, in.B, n, rgb_map, depth, weights, ms, *bga);
  else
    hipLaunchKernelGGL((composite_kernel<VEC, MERGED, STAGE>), dim3(p.grid), dim3(p.block), p.lds, s, rgb, sigma, in.z,
                       in.B, n, rgb_map, depth, weights, ms);
}

int launch_composite(const CompositeSamples& in, float* rgb_map, float* depth, float* weights, const CompositeBg* bga,
                     hipStream_t s) {
  const CompositePlan p = composite_forward_plan(in.B, in.N, in.Nf, in.merged, in.rgb, in.sigma, in.z, weights, bga);
  if (p.action == CompositePlan::kSkip) return NERF_OK;
  switch (p.vec | p.stage << 1 | p.merged << 2) {   // (STAGE is a merged variant)
    case 0: launch_variant<false, false>(p, in, rgb_map, depth, weights, bga, s); break;
    case 1: launch_variant<true, false>(p, in, rgb_map, depth, weights, bga, s); break;
    case 4: launch_variant<false, true>(p, in, rgb_map, depth, weights, bga, s); break;
    case 5: launch_variant<true, true>(p, in, rgb_map, depth, weights, bga, s); break;
    case 6: launch_variant<false, true, true>(p, in, rgb_map, depth, weights, bga, s); break;
    case 7: launch_variant<true, true, true>(p, in, rgb_map, depth, weights, bga, s); break;
  }
  return check_launch(p.name);
}

}  // namespace nerf
