// What decides a composite launch, forward (composite.hip) and backward (composite_bwd.hip), as pure
// host functions of the shape, the pointer values and the options: the kernel variant, its grid, block
// and dynamic LDS, or a refusal.  No HIP types and no globals, so a plain host compiler builds it:
// tests/composite_plan_dump.cpp prints the plans over a table of cases and tests/test_composite_plan.py
// checks them against the rules written out there.  VEC is the choice that matters most: it means
// 16-byte loads and stores, and on a pointer that is not 16-byte aligned those are an illegal access.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace nerf {

constexpr int kStageT = 256;           // merged forward: rows of up to this many samples are staged in LDS
constexpr int kMergedBwdMaxT = 1280;   // merged backward: N <= 256, Nf <= 1024 (the resampler's limits)

struct CompositePlan {
  enum Action { kSkip, kLaunch, kRefuse } action;   // kSkip: an empty batch, NERF_OK without a launch
  bool vec, merged, stage;   // the kernel's template arguments (the backward kernels have no VEC / STAGE)
  bool alt;                  // forward: composite_bg_kernel; backward: the _acc kernels
  unsigned grid, block;
  size_t lds;                // dynamic LDS bytes
  const char* name;          // what check_launch reports
  bool per_sample;           // backward: the _w kernels (alt is set too)
};

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// Forward over B rays of N samples (merged: N coarse + Nf fine, z = z_all, and rgb / sigma are not looked
// at: the kernel gathers single floats through the map).  weights is nullable.
inline CompositePlan composite_forward_plan(int64_t B, int N, int Nf, bool merged, const void* rgb, const void* sigma,
                                            const void* z, const void* weights, bool bg) {
  CompositePlan p{};
  p.merged = merged, p.alt = bg;
  p.name = merged ? (bg ? "composite_bg_kernel (merged)" : "composite_kernel (merged)")
                  : (bg ? "composite_bg_kernel" : "composite_kernel");
  if (B == 0) return p;
  p.action = CompositePlan::kLaunch;
  const int T = merged ? N + Nf : N;
  p.vec = T % 4 == 0 && (merged || (aligned16(rgb) && aligned16(sigma))) && aligned16(z) && aligned16(weights);
  p.stage = merged && T <= kStageT;   // 8 rays per block, one (r, g, b, sigma) quad per sample
  const int rays = p.stage ? 8 : 16;
  p.grid = (unsigned)((B + rays - 1) / rays), p.block = 16 * rays;
  p.lds = p.stage ? (size_t)8 * T * 16 : 0;
  return p;
}

// Backward: one wave per ray.  The merged kernel keeps a ray's T = N + Nf quads in LDS: 4 rays per
// block up to T = 768 and 2 beyond (40 KB at kMergedBwdMaxT).
// per_sample (with acc): the _w kernels, the _acc ones with a per-sample gradient of the weights; the
// same grid, block and LDS.
inline CompositePlan composite_backward_plan(int64_t B, int N, int Nf, bool merged, bool acc, bool per_sample = false) {
  CompositePlan p{};
  p.merged = merged, p.alt = acc, p.per_sample = acc && per_sample;
  p.name = merged ? (acc ? "composite_merged_backward_acc_kernel" : "composite_merged_backward_kernel")
                  : (acc ? "composite_backward_acc_kernel" : "composite_backward_kernel");
  if (p.per_sample) p.name = merged ? "composite_merged_backward_w_kernel" : "composite_backward_w_kernel";
  if (B == 0) return p;
  const int T = N + Nf;
  if (merged && (N < 1 || Nf < 1 || T > kMergedBwdMaxT)) {
    p.action = CompositePlan::kRefuse;
    return p;
  }
  p.action = CompositePlan::kLaunch;
  const int rpb = !merged || T <= 768 ? 4 : 2;   // rays per block: at most 48 KB of LDS
  p.grid = (unsigned)((B + rpb - 1) / rpb), p.block = 64 * rpb;
  p.lds = merged ? (size_t)rpb * T * 16 : 0;
  return p;
}

}  // namespace nerf
