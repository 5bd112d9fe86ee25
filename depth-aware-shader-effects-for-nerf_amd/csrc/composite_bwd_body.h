// The bodies of composite_bwd.hip's two kernels, included once per variant:
//   COMPOSITE_BWD_ACC 0: composite_backward_kernel and composite_merged_backward_kernel;
//   COMPOSITE_BWD_ACC 1: composite_backward_acc_kernel and composite_merged_backward_acc_kernel, the
//     same text with a per-ray upstream gradient g_acc of the opacity acc = sum w (nullable = 0; it is
//     added to every dw of the ray) and bd, the background depth of the forward: when
//     bd is not NaN the depth is S + k bd, k = max(0, 1 - acc), and its term is gd (z_s - bd) where
//     k > 0 and gd z_s where k == 0.  Same arithmetic order: double scans, d sigma rounded once.  With
//     g_acc null or zero and bd NaN every operation is the plain kernel's: the same bits.
//   COMPOSITE_BWD_ACC 1 with COMPOSITE_BWD_W 1: composite_backward_w_kernel and
//     composite_merged_backward_w_kernel, the _acc text with a per-sample upstream gradient g_w of the
//     weights ((B,N); merged: (B,N+Nf) in merged order; nullable = 0), added to the sample's dw right
//     after g_acc.  With g_w null or zero every operation is the _acc kernel's.
#ifndef COMPOSITE_BWD_W
#define COMPOSITE_BWD_W 0
#endif
__global__ void __launch_bounds__(256)
#if COMPOSITE_BWD_W
composite_backward_w_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma,
                            const float* __restrict__ zv, const float* __restrict__ rgb_map,
                            const float* __restrict__ target, const float* __restrict__ grad_map,
                            const float* __restrict__ grad_depth, int64_t B, int N, float scale,
                            float* __restrict__ dsigma, float* __restrict__ drgb, float* __restrict__ sq_err,
                            const float* __restrict__ g_acc, float bd, const float* __restrict__ g_w) {
#elif COMPOSITE_BWD_ACC
composite_backward_acc_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma,
                              const float* __restrict__ zv, const float* __restrict__ rgb_map,
                              const float* __restrict__ target, const float* __restrict__ grad_map,
                              const float* __restrict__ grad_depth, int64_t B, int N, float scale,
                              float* __restrict__ dsigma, float* __restrict__ drgb, float* __restrict__ sq_err,
                              const float* __restrict__ g_acc, float bd) {
#else
composite_backward_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma, const float* __restrict__ zv,
                          const float* __restrict__ rgb_map, const float* __restrict__ target,
                          const float* __restrict__ grad_map, const float* __restrict__ grad_depth, int64_t B, int N,
                          float scale, float* __restrict__ dsigma, float* __restrict__ drgb,
                          float* __restrict__ sq_err) {
#endif
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
#if COMPOSITE_BWD_ACC
  const float ga = g_acc ? g_acc[r] : 0.0f;      // d loss / d acc: added to every dw of the ray
  const bool bg_depth = bd == bd;                // depth = S + k bd instead of S / (A + 1e-10)
#endif
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
#if COMPOSITE_BWD_ACC
      if (bg_depth) {                            // A as the forward rounds it: the sum of its float weights
        ws += (double)(alpha * (float)(carry * excl));
      } else
#endif
      {
        const double w = (double)alpha * (carry * excl);
        wz += w * (double)z;
        ws += w;
      }
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
#if COMPOSITE_BWD_ACC
    if (bg_depth) {                              // d depth / d w_s = z_s - bd where k > 0, z_s where k == 0
      dinv = 1.0;
      dmean = fmaxf(0.0f, 1.0f - (float)ws) > 0.0f ? (double)bd : 0.0;
    } else
#endif
    {
      const double den = ws + (double)1e-10f;
      dinv = 1.0 / den;
      dmean = wz * dinv;
    }
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
#if COMPOSITE_BWD_ACC
      if (ga != 0.0f) dw += (double)ga;
#endif
#if COMPOSITE_BWD_W
      const float gw = g_w ? g_w[base + s] : 0.0f;   // d loss / d w_s from outside the composite
      if (gw != 0.0f) dw += (double)gw;
#endif
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

__global__ void __launch_bounds__(256)
#if COMPOSITE_BWD_W
composite_merged_backward_w_kernel(
#elif COMPOSITE_BWD_ACC
composite_merged_backward_acc_kernel(
#else
composite_merged_backward_kernel(
#endif
    const float* __restrict__ rgb_c, const float* __restrict__ sigma_c,
                                 const float* __restrict__ rgb_f, const float* __restrict__ sigma_f,
                                 const uint16_t* __restrict__ src, const float* __restrict__ zv,
                                 const float* __restrict__ rgb_map, const float* __restrict__ target,
                                 const float* __restrict__ grad_map, const float* __restrict__ grad_depth, int64_t B,
                                 int N, int Nf, float scale, int accumulate, float* dsigma_c, float* drgb_c,
                                 float* __restrict__ dsigma_f, float* __restrict__ drgb_f,
                                 float* __restrict__ sq_err
#if COMPOSITE_BWD_ACC
                                 , const float* __restrict__ g_acc, float bd
#endif
#if COMPOSITE_BWD_W
                                 , const float* __restrict__ g_w
#endif
                                 ) {
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
#if COMPOSITE_BWD_ACC
  const float ga = g_acc ? g_acc[r] : 0.0f;      // d loss / d acc: added to every dw of the ray
  const bool bg_depth = bd == bd;                // depth = S + k bd instead of S / (A + 1e-10)
#endif
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
#if COMPOSITE_BWD_ACC
      if (bg_depth) {                            // A as the forward rounds it: the sum of its float weights
        ws += (double)(alpha * (float)(carry * excl));
      } else
#endif
      {
        const double w = (double)alpha * (carry * excl);
        wz += w * (double)z;
        ws += w;
      }
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
#if COMPOSITE_BWD_ACC
    if (bg_depth) {                              // d depth / d w_s = z_s - bd where k > 0, z_s where k == 0
      dinv = 1.0;
      dmean = fmaxf(0.0f, 1.0f - (float)ws) > 0.0f ? (double)bd : 0.0;
    } else
#endif
    {
      const double den = ws + (double)1e-10f;
      dinv = 1.0 / den;
      dmean = wz * dinv;
    }
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
#if COMPOSITE_BWD_ACC
      if (ga != 0.0f) dw += (double)ga;
#endif
#if COMPOSITE_BWD_W
      const float gw = g_w ? g_w[base + s] : 0.0f;   // d loss / d w_s from outside the composite
      if (gw != 0.0f) dw += (double)gw;
#endif
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
