// Training path, stage 1 of the backward (BASELINE config 5): the composite
// backward.  Reference: src/train.py:77-92 (MSE against the target rgb :87, loss.backward())
// through src/render.py:56-80.
//
//   composite_backward_kernel   d loss / d(sigma, rgb) per sample from d loss / d rgb_map (and
//                               d depth_map), one wave per ray, reverse double-precision scan
//   composite_merged_backward_kernel   the same over the N + Nf merged samples of the hierarchical
//                               step, gathered from and written back to the coarse and fine rows
//                               through LDS
#include "train_internal.h"

namespace nerf {

// ---------------------------------------------------------------------------- composite bwd
// render.py:56-80 differentiated.  With g = d loss / d rgb_map (3), per sample s of a ray:
//   drgb_s = w_s g;  dw_s = g . rgb_s;  T_s = prod_{j<s} f_j, f_j = 1 - a_j + 1e-10
//   d a_s = dw_s T_s - (1/f_s) sum_{t>s} dw_t w_t;   d sigma_s = d a_s * dist_s * exp(-sigma_s dist_s)
// The training loss is mean((rgb_map - target)^2) over B x 3 (train.py:87): g = 2 (rgb_map - target)/(3B),
// sq_err[r] = sum_c (rgb_map - target)^2 for the loss value.  Given an arbitrary upstream gradient
// instead (autograd: grad_map (B,3) for rgb_map, grad_depth (B) for depth_map, each nullable = 0),
// g = grad_map[r] and the depth term of depth = S / (A + 1e-10), S = sum w z, A = sum w (:80) adds
//   dw_s += gd (z_s - S / (A + 1e-10)) / (A + 1e-10)
// with S and A re-accumulated in the forward pass.  dw, T, w and d a stay in double and d sigma is
// rounded once: d a_s is a difference of two terms of the size of dw (an empty sample in front of a
// surface: dw_s - sum dw_t w_t), and float roundings of dw, w and T there put d sigma twice as far from
// the float64 gradient as torch's fp32 autograd (tests/test_gpu_degenerate_rays.py).  drgb is the
// forward's float weight times g.
__global__ void __launch_bounds__(256)
composite_backward_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma, const float* __restrict__ zv,
                          const float* __restrict__ rgb_map, const float* __restrict__ target,
                          const float* __restrict__ grad_map, const float* __restrict__ grad_depth, int64_t B, int N,
                          float scale, float* __restrict__ dsigma, float* __restrict__ drgb,
                          float* __restrict__ sq_err) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const int64_t base = r * N;
  float g[3], se = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (target) {
      const float e = rgb_map[3 * r + c] - target[3 * r + c];
      g[c] = scale * e;
      se += e * e;
    } else {
      g[c] = grad_map ? grad_map[3 * r + c] : 0.0f;
    }
  }
  const float gd = grad_depth ? grad_depth[r] : 0.0f;
  if (lane == 0 && sq_err) sq_err[r] = se;
  if (N == 1) {                       // the reference's per-sample tensors are empty (render.py:56-58)
    if (lane == 0) {
      dsigma[base] = 0.0f;
      drgb[3 * base] = drgb[3 * base + 1] = drgb[3 * base + 2] = 0.0f;
    }
    return;
  }
  // pass 1 (forward order): transmittance prefix, carried across 64-sample chunks (and, with a
  // depth gradient, S and A)
  // pass 2 (reverse order): suffix sums of dw*w; done chunk by chunk from the end, recomputing
  // each chunk's T from the stored chunk-start prefixes.
  const int nchunk = (N + 63) / 64;
  __shared__ double carry_lds[4][64]; // T at each chunk start (N <= 4096)
  double* carry_chunk = carry_lds[threadIdx.x >> 6];
  double carry = 1.0, wz = 0.0, ws = 0.0;
  for (int c = 0; c < nchunk; ++c) {
    const int s = c * 64 + lane;
    double f = 1.0;
    float alpha = 0.0f, z = 0.0f;
    if (s < N) {
      z = zv[base + s];
      const float dist = (s + 1 < N) ? zv[base + s + 1] - z : 1e-3f;
      alpha = 1.0f - expf_rn(-sigma[base + s] * dist);
      f = (double)((1.0f - alpha) + 1e-10f);
    }
    double incl = f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double up = __shfl_up(incl, off);
      if (lane >= off) incl *= up;
    }
    if (gd != 0.0f) {
      double excl = __shfl_up(incl, 1);
      if (lane == 0) excl = 1.0;
      const double w = (double)alpha * (carry * excl);
      wz += w * (double)z;
      ws += w;
    }
    if (lane == 0) carry_chunk[c] = carry;
    carry *= __shfl(incl, 63);
  }
  double dinv = 0.0, dmean = 0.0;    // 1 / (A + 1e-10), S / (A + 1e-10)
  if (gd != 0.0f) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      wz += __shfl_xor(wz, off);
      ws += __shfl_xor(ws, off);
    }
    const double den = ws + (double)1e-10f;
    dinv = 1.0 / den;
    dmean = wz * dinv;
  }
  __builtin_amdgcn_wave_barrier();
  double suffix = 0.0;                // sum_{t > current chunk} dw_t w_t
  for (int c = nchunk - 1; c >= 0; --c) {
    const int s = c * 64 + lane;
    const bool valid = s < N;
    float alpha = 0.0f, dist = 0.0f, e = 1.0f, fs = 1.0f, sg = 0.0f, z = 0.0f;
    double f = 1.0;
    if (valid) {
      z = zv[base + s];
      dist = (s + 1 < N) ? zv[base + s + 1] - z : 1e-3f;
      sg = sigma[base + s];
      e = expf_rn(-sg * dist);
      alpha = 1.0f - e;
      fs = (1.0f - alpha) + 1e-10f;
      f = (double)fs;
    }
    double incl = f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double up = __shfl_up(incl, off);
      if (lane >= off) incl *= up;
    }
    double excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 1.0;
    const double T = carry_chunk[c] * excl;
    const float w = alpha * (float)T;                      // the forward's weight (composite.hip)
    double dw = 0.0;
    if (valid) {
      const int64_t e3 = 3 * (base + s);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        dw += (double)g[k] * (double)rgb[e3 + k];
        drgb[e3 + k] = w * g[k];
      }
      if (gd != 0.0f) dw += (double)gd * ((double)z - dmean) * dinv;
    }
    // exclusive suffix sum of dw*w inside the chunk, plus the chunks after it
    double v = valid ? dw * ((double)alpha * T) : 0.0;
    double incl_rev = v;                                   // inclusive suffix within the chunk
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double dn = __shfl_down(incl_rev, off);
      if (lane + off < 64) incl_rev += dn;
    }
    const double excl_rev = incl_rev - v + suffix;
    if (valid) {
      const double da = dw * T - excl_rev / (double)fs;
      dsigma[base + s] = (float)(da * (double)dist * (double)e);
    }
    suffix += __shfl(incl_rev, 0);
  }
}

int launch_composite_backward(const float* rgb, const float* sigma, const float* z, const float* rgb_map,
                              const float* target, const float* grad_map, const float* grad_depth, int64_t B, int N,
                              float scale, float* dsigma, float* drgb, float* sq_err, hipStream_t s) {
  if (B == 0) return NERF_OK;
  hipLaunchKernelGGL(composite_backward_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, rgb, sigma, z,
                     rgb_map, target, grad_map, grad_depth, B, N, scale, dsigma, drgb, sq_err);
  return check_launch("composite_backward_kernel");
}

// ------------------------------------------------------------------- merged composite bwd
// The backward of composite.hip's MERGED composite (the hierarchical step): position
// p of ray r's T = N + Nf merged samples is sample e = src[r T + p] of cat[coarse, fine] (e < N: row
// r N + e of the coarse arrays, else row r Nf + e - N of the fine ones), z from z_all.  The
// arithmetic is composite_backward_kernel's, operation for operation and in its scan order (one
// wave per ray, 64 positions per chunk), so on the same merged rows the results are the same bits.
//
// Memory: the ray's coarse and fine (rgb, sigma) rows are first copied into LDS as one
// (r, g, b, sigma) quad per cat index with whole-row coalesced loads (the route of composite.hip's
// STAGE, which measured gathering from global memory at 6x the cost); the scans gather from there,
// write each sample's (drgb, dsigma) over the quad it came from (a cat index occurs once per ray,
// and a quad is last read when its sample's results are formed), and the quads go back to the split
// rows as whole coalesced rows.  Every output element has one writer.  Coarse rows take in + term
// when `accumulate` is set (the coarse composite's own term is already there), fine rows are always
// written.  LDS: 16 T bytes per ray; the launcher puts 4 rays in a block up to T = 768 and 2 beyond
// (40 KB at kMergedBwdMaxT).
constexpr int kMergedBwdMaxT = 1280;          // N <= 256, Nf <= 1024 (the resampler's limits)
constexpr int kMergedBwdChunks = kMergedBwdMaxT / 64;

__global__ void __launch_bounds__(256)
composite_merged_backward_kernel(const float* __restrict__ rgb_c, const float* __restrict__ sigma_c,
                                 const float* __restrict__ rgb_f, const float* __restrict__ sigma_f,
                                 const uint16_t* __restrict__ src, const float* __restrict__ zv,
                                 const float* __restrict__ rgb_map, const float* __restrict__ target,
                                 const float* __restrict__ grad_map, const float* __restrict__ grad_depth, int64_t B,
                                 int N, int Nf, float scale, int accumulate, float* dsigma_c, float* drgb_c,
                                 float* __restrict__ dsigma_f, float* __restrict__ drgb_f,
                                 float* __restrict__ sq_err) {
  extern __shared__ f32x4 quads[];    // [rays per block][T]
  __shared__ double carry_lds[4][kMergedBwdChunks];   // T at each chunk start
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * ((int)blockDim.x >> 6) + wid;
  if (r >= B) return;                 // (no block-wide barrier below: a wave owns its ray's LDS)
  const int T = N + Nf;
  const int64_t base = r * T, base_c = r * N, base_f = r * Nf;
  f32x4* rq = quads + wid * T;
  for (int e = lane; e < T; e += 64) {
    const bool crs = e < N;
    const int64_t at = crs ? base_c + e : base_f + (e - N);
    const float* cs = crs ? rgb_c : rgb_f;
    rq[e] = f32x4{cs[3 * at], cs[3 * at + 1], cs[3 * at + 2], (crs ? sigma_c : sigma_f)[at]};
  }
  float g[3], se = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (target) {
      const float e = rgb_map[3 * r + c] - target[3 * r + c];
      g[c] = scale * e;
      se += e * e;
    } else {
      g[c] = grad_map ? grad_map[3 * r + c] : 0.0f;
    }
  }
  const float gd = grad_depth ? grad_depth[r] : 0.0f;
  if (lane == 0 && sq_err) sq_err[r] = se;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // pass 1 (forward order) and pass 2 (reverse order) as in composite_backward_kernel
  const int nchunk = (T + 63) / 64;
  double* carry_chunk = carry_lds[wid];
  double carry = 1.0, wz = 0.0, ws = 0.0;
  for (int c = 0; c < nchunk; ++c) {
    const int s = c * 64 + lane;
    double f = 1.0;
    float alpha = 0.0f, z = 0.0f;
    if (s < T) {
      z = zv[base + s];
      const float dist = (s + 1 < T) ? zv[base + s + 1] - z : 1e-3f;
      alpha = 1.0f - expf_rn(-rq[src[base + s]][3] * dist);
      f = (double)((1.0f - alpha) + 1e-10f);
    }
    double incl = f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double up = __shfl_up(incl, off);
      if (lane >= off) incl *= up;
    }
    if (gd != 0.0f) {
      double excl = __shfl_up(incl, 1);
      if (lane == 0) excl = 1.0;
      const double w = (double)alpha * (carry * excl);
      wz += w * (double)z;
      ws += w;
    }
    if (lane == 0) carry_chunk[c] = carry;
    carry *= __shfl(incl, 63);
  }
  double dinv = 0.0, dmean = 0.0;    // 1 / (A + 1e-10), S / (A + 1e-10)
  if (gd != 0.0f) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      wz += __shfl_xor(wz, off);
      ws += __shfl_xor(ws, off);
    }
    const double den = ws + (double)1e-10f;
    dinv = 1.0 / den;
    dmean = wz * dinv;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double suffix = 0.0;                // sum_{t > current chunk} dw_t w_t
  for (int c = nchunk - 1; c >= 0; --c) {
    const int s = c * 64 + lane;
    const bool valid = s < T;
    float alpha = 0.0f, dist = 0.0f, e = 1.0f, fs = 1.0f, z = 0.0f;
    double f = 1.0;
    int at = 0;                       // the sample's cat index
    f32x4 q = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
      z = zv[base + s];
      dist = (s + 1 < T) ? zv[base + s + 1] - z : 1e-3f;
      at = (int)src[base + s];
      q = rq[at];
      e = expf_rn(-q[3] * dist);
      alpha = 1.0f - e;
      fs = (1.0f - alpha) + 1e-10f;
      f = (double)fs;
    }
    double incl = f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double up = __shfl_up(incl, off);
      if (lane >= off) incl *= up;
    }
    double excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 1.0;
    const double Tr = carry_chunk[c] * excl;
    const float w = alpha * (float)Tr;                     // the forward's weight (composite.hip)
    double dw = 0.0;
    f32x4 out = {0.0f, 0.0f, 0.0f, 0.0f};                  // (drgb, dsigma)
    if (valid) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        dw += (double)g[k] * (double)q[k];
        out[k] = w * g[k];
      }
      if (gd != 0.0f) dw += (double)gd * ((double)z - dmean) * dinv;
    }
    double v = valid ? dw * ((double)alpha * Tr) : 0.0;
    double incl_rev = v;                                   // inclusive suffix within the chunk
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double dn = __shfl_down(incl_rev, off);
      if (lane + off < 64) incl_rev += dn;
    }
    const double excl_rev = incl_rev - v + suffix;
    if (valid) {
      const double da = dw * Tr - excl_rev / (double)fs;
      out[3] = (float)(da * (double)dist * (double)e);
      rq[at] = out;
    }
    suffix += __shfl(incl_rev, 0);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int e = lane; e < T; e += 64) {
    const f32x4 q = rq[e];
    if (e < N) {
      const int64_t at = base_c + e;
      if (accumulate) {
        dsigma_c[at] = dsigma_c[at] + q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) drgb_c[3 * at + k] = drgb_c[3 * at + k] + q[k];
      } else {
        dsigma_c[at] = q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) drgb_c[3 * at + k] = q[k];
      }
    } else {
      const int64_t at = base_f + (e - N);
      dsigma_f[at] = q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) drgb_f[3 * at + k] = q[k];
    }
  }
}

int launch_composite_merged_backward(const float* rgb_c, const float* sigma_c, const float* rgb_f,
                                     const float* sigma_f, const uint16_t* src, const float* z_all,
                                     const float* rgb_map, const float* target, const float* grad_map,
                                     const float* grad_depth, int64_t B, int N, int Nf, float scale, int accumulate,
                                     float* dsigma_c, float* drgb_c, float* dsigma_f, float* drgb_f, float* sq_err,
                                     hipStream_t s) {
  if (B == 0) return NERF_OK;
  const int T = N + Nf;
  if (N < 1 || Nf < 1 || T > kMergedBwdMaxT)
    return set_error(NERF_ERR_UNSUPPORTED, "composite_merged_backward: N=%d Nf=%d (N + Nf <= %d)", N, Nf, kMergedBwdMaxT);
  const int rpb = T <= 768 ? 4 : 2;   // rays per block: at most 48 KB of LDS
  const size_t lds = (size_t)rpb * T * sizeof(f32x4);
  hipLaunchKernelGGL(composite_merged_backward_kernel, dim3((unsigned)((B + rpb - 1) / rpb)), dim3(64 * rpb), lds, s,
                     rgb_c, sigma_c, rgb_f, sigma_f, src, z_all, rgb_map, target, grad_map, grad_depth, B, N, Nf, scale,
                     accumulate, dsigma_c, drgb_c, dsigma_f, drgb_f, sq_err);
  return check_launch("composite_merged_backward_kernel");
}

// dst[i] += src[i] over up to 25 segments (the hierarchical step's second gradient set into the
// first): one writer per element, a single float add, so the sum has one fixed order
struct AddSegs {
  float* dst[25];
  const float* src[25];
  int n[25];
};
__global__ void __launch_bounds__(256) add_segments_kernel(AddSegs a) {
  const int seg = blockIdx.y;
  float* __restrict__ d = a.dst[seg];
  const float* __restrict__ x = a.src[seg];
  const int n = a.n[seg];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] = d[i] + x[i];
}

int launch_add_segments(float* const* dst, const float* const* src, const size_t* n, int count, hipStream_t s) {
  if (count < 1 || count > 25) return set_error(NERF_ERR_BAD_ARG, "add_segments: count=%d", count);
  AddSegs a{};
  size_t most = 0;
  for (int i = 0; i < count; ++i) {
    a.dst[i] = dst[i], a.src[i] = src[i], a.n[i] = (int)n[i];
    most = n[i] > most ? n[i] : most;
  }
  if (most == 0) return NERF_OK;
  const unsigned gx = (unsigned)((most + 255) / 256 < 64 ? (most + 255) / 256 : 64);
  hipLaunchKernelGGL(add_segments_kernel, dim3(gx, (unsigned)count), dim3(256), 0, s, a);
  return check_launch("add_segments_kernel");
}

}  // namespace nerf
