// The body of composite.hip's kernels, included once per kernel:
//   COMPOSITE_BG 0: composite_kernel, the composite of nerf_composite and nerf_render_rays;
//   COMPOSITE_BG 1: composite_bg_kernel, the same text with the opacity output and the background
//     blend in the last lane's epilogue (composite.hip).  Everything before the
//     epilogue, the weights included, is the plain kernel's, instruction for instruction in source order.
template <bool VEC, bool MERGED, bool STAGE = false>
__global__ void __launch_bounds__(256)
#if COMPOSITE_BG
composite_bg_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma, const float* __restrict__ zv,
                    int64_t B, int N, float* __restrict__ rgb_map, float* __restrict__ depth_map,
                    float* __restrict__ weights, MergedSrc ms, CompositeBg bga) {
#else
composite_kernel(const float* __restrict__ rgb, const float* __restrict__ sigma, const float* __restrict__ zv,
                 int64_t B, int N, float* __restrict__ rgb_map, float* __restrict__ depth_map,
                 float* __restrict__ weights, MergedSrc ms) {
#endif
  extern __shared__ f32x4 quads[];   // STAGE: [8 rays][T]
  const int k = threadIdx.x & 15;
  const int rpb = (int)blockDim.x >> 4;                       // rays per block: 16, or 8 when STAGE
  const int64_t r = (int64_t)blockIdx.x * rpb + (threadIdx.x >> 4);
  const bool ray = r < B;          // rows past B run on with no samples (the DPP stays inside a row)
  const int64_t base = ray ? r * N : 0;
  if constexpr (STAGE) {           // every thread reaches the barrier
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int nr = (int)(B - r0 < rpb ? B - r0 : rpb);
    const int nc = ms.nc, nf = ms.nf;
    for (int i = threadIdx.x; i < nr * N; i += (int)blockDim.x) {   // quad i: ray i / T, cat index i % T
      const int rr = i / N, e = i - rr * N;
      const bool crs = e < nc;
      const int64_t at = crs ? (r0 + rr) * nc + e : (r0 + rr) * nf + (e - nc);
      const float* cs = crs ? ms.rgb_c : ms.rgb_f;
      quads[i] = f32x4{cs[3 * at], cs[3 * at + 1], cs[3 * at + 2], (crs ? ms.sigma_c : ms.sigma_f)[at]};
    }
    __syncthreads();
  }
  const f32x4* rq = quads + (threadIdx.x >> 4) * N;   // STAGE: this ray's quads
  if (ray && N == 1 && weights && k == 0) weights[base] = 0.0f;
  const int n_eff = ray && N > 1 ? N : 0;
  double carry = 1.0;
  double acc_r = 0.0, acc_g = 0.0, acc_b = 0.0, acc_wz = 0.0, acc_w = 0.0;
  for (int c0 = 0; c0 < n_eff; c0 += 64) {
    const int s0 = c0 + 4 * k;
    float z[5], sg[4], c[12];
    if constexpr (MERGED) {
      int e[4];
      if (VEC && s0 + 4 <= n_eff) {    // z and the 4 slots' sources as one 16- and one 8-byte load
        const f32x4 zq = *reinterpret_cast<const f32x4*>(zv + base + s0);
        const uint2 sq = *reinterpret_cast<const uint2*>(ms.src + base + s0);
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = zq[j];
        e[0] = (int)(sq.x & 0xffffu), e[1] = (int)(sq.x >> 16), e[2] = (int)(sq.y & 0xffffu), e[3] = (int)(sq.y >> 16);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool v = s0 + j < n_eff;
          z[j] = v ? zv[base + s0 + j] : 0.0f;
          e[j] = v ? (int)ms.src[base + s0 + j] : -1;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool v = e[j] >= 0;
        f32x4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (STAGE) {
          if (v) q = rq[e[j]];
        } else if (v) {
          const bool crs = e[j] < ms.nc;
          const int64_t at = crs ? r * ms.nc + e[j] : r * ms.nf + (e[j] - ms.nc);
          const float* cs = crs ? ms.rgb_c : ms.rgb_f;
          q = f32x4{cs[3 * at], cs[3 * at + 1], cs[3 * at + 2], (crs ? ms.sigma_c : ms.sigma_f)[at]};
        }
        sg[j] = q[3];
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) c[3 * j + c3] = q[c3];
      }
    } else if (VEC && s0 + 4 <= n_eff) {
      const f32x4 zq = *reinterpret_cast<const f32x4*>(zv + base + s0);
      const f32x4 sq = *reinterpret_cast<const f32x4*>(sigma + base + s0);
#pragma unroll
      for (int j = 0; j < 4; ++j) z[j] = zq[j], sg[j] = sq[j];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const f32x4 cq = *reinterpret_cast<const f32x4*>(rgb + 3 * (base + s0) + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[4 * q + j] = cq[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool v = s0 + j < n_eff;
        z[j] = v ? zv[base + s0 + j] : 0.0f;
        sg[j] = v ? sigma[base + s0 + j] : 0.0f;
#pragma unroll
        for (int q = 0; q < 3; ++q) c[3 * j + q] = v ? rgb[3 * (base + s0 + j) + q] : 0.0f;
      }
    }
    z[4] = s0 + 4 < n_eff ? zv[base + s0 + 4] : 0.0f;
    float alpha[4];
    double f[4], lane_prod = 1.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = s0 + j;
      alpha[j] = 0.0f;
      f[j] = 1.0;
      if (s < n_eff) {
        const float dist = (s + 1 < N) ? z[j + 1] - z[j] : 1e-3f;
        alpha[j] = 1.0f - expf_rn(-sg[j] * dist);
        f[j] = (double)((1.0f - alpha[j]) + 1e-10f);
      }
      lane_prod *= f[j];
    }
    const double incl = row_scan_mul(lane_prod);
    double pre = carry * row_shr<1>(incl, 1.0);      // product of every factor before this lane's first
    carry *= __shfl(incl, 15, 16);
    float w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = alpha[j] * (float)pre;                  // 0 past the ray's end (alpha = 0)
      pre *= f[j];
      acc_r += (double)(w[j] * c[3 * j]);
      acc_g += (double)(w[j] * c[3 * j + 1]);
      acc_b += (double)(w[j] * c[3 * j + 2]);
      acc_wz += (double)(w[j] * z[j]);
      acc_w += (double)w[j];
    }
    if (weights) {
      if (VEC && s0 + 4 <= n_eff) {
        *reinterpret_cast<f32x4*>(weights + base + s0) = f32x4{w[0], w[1], w[2], w[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (s0 + j < n_eff) weights[base + s0 + j] = w[j];
      }
    }
  }
  acc_r = row_scan_add(acc_r);
  acc_g = row_scan_add(acc_g);
  acc_b = row_scan_add(acc_b);
  acc_wz = row_scan_add(acc_wz);
  acc_w = row_scan_add(acc_w);
#if COMPOSITE_BG
  if (ray && k == 15) {
    const float acc = (float)acc_w;
    const float kb = fmaxf(0.0f, 1.0f - acc);
    float out[3] = {(float)acc_r, (float)acc_g, (float)acc_b};
    if (bga.bg) {
      const float* b = bga.bg + (int64_t)bga.stride * r;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float t = kb * b[q];       // the product rounded, then the sum
        out[q] = out[q] + t;
      }
    }
    rgb_map[3 * r] = out[0];
    rgb_map[3 * r + 1] = out[1];
    rgb_map[3 * r + 2] = out[2];
    if (bga.bd != bga.bd) {              // NaN: the normalised depth
      depth_map[r] = (float)acc_wz / (acc + 1e-10f);
    } else {
      const float t = kb * bga.bd;
      depth_map[r] = (float)acc_wz + t;
    }
    if (bga.acc_map) bga.acc_map[r] = acc;
  }
#else
  if (ray && k == 15) {
    rgb_map[3 * r] = (float)acc_r;
    rgb_map[3 * r + 1] = (float)acc_g;
    rgb_map[3 * r + 2] = (float)acc_b;
    depth_map[r] = (float)acc_wz / ((float)acc_w + 1e-10f);
  }
#endif
}
