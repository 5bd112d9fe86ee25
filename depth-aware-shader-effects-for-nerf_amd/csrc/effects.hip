// Depth-aware post effects of the reference's PostProcessor (src/post_processor.py) on the GPU,
// the two effects that read the depth map, Fog (:451-493) and Toon Shader
// (:64-117), plus the depth normalisation run.py applies before them (run.py:248).
//
// Images are the reference's uint8 HxWx3 RGB frames; depth is fp32 HxW (a channel stride lets a
// HxWxC depth use its first channel, as post_processor.py:474-475 does).  The arithmetic follows
// numpy's float32 semantics of the reference expressions (Python scalars cast to float32, one
// rounding per operation, astype(uint8) truncating after the clip).  The cv2 operations of Toon
// (bilateralFilter, Sobel, dilate, cvtColor, Laplacian) are restated from OpenCV 4's algorithms:
// cv2 is not installed here, so that part is pinned to oracle/post_oracle.py, not to cv2.
//
// Every pass is a per-pixel HBM-bound kernel on an 800x800 frame (a few MB): the work is in
// global reductions (max/min for the normalisations, ordered-integer atomics, exact in any order)
// and 3x3 / 9x9 stencils.
//
// The second half of the file adds Vignette, Cross Processing, Film Grain, Hologram, Posterize,
// Bloom and Pencil Sketch.  Their numpy steps follow numpy 2's promotion rules operation for
// operation (a Python float with a uint8 array is float64, with a float32 array float32, so
// Vignette's distance field, Posterize's edge blend and Pencil Sketch's masked blend are float64
// on the device too) and are pinned to the reference's own code by fixture F10
// (tests/golden/make_effects_golden.py).  Their cv2 steps are parity unpinned, restated in
// tests/effects_restated.py: cvtColor/Laplacian (exact in integers), Sobel (as Toon's),
// cv2.divide, and two that are definitions of this project rather than OpenCV's code path:
// GaussianBlur (float32 separable filter below; cv2's 8-bit path uses fixed-point coefficients and
// may differ by a count) and addWeighted (float32 multiply, add, round half to even).
// np.percentile (Pencil Sketch's background mask) is an exact radix select on the device.
#include <math.h>
#include <float.h>

#include "common.h"

namespace nerf {

// Total order on floats as unsigned integers (max/min by atomics are then exact).
__device__ __forceinline__ unsigned f2ord(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// mm[0] = max, mm[1] = min (ordered) of x[i*stride], i < n.  mm preset to {0, ~0}.
__global__ void __launch_bounds__(256) minmax_kernel(const float* __restrict__ x, int64_t n, int64_t stride,
                                                      unsigned* __restrict__ mm) {
  unsigned mx = 0u, mn = 0xffffffffu;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned o = f2ord(x[i * stride]);
    mx = max(mx, o);
    mn = min(mn, o);
  }
  for (int off = 32; off > 0; off >>= 1) {
    mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
    mn = min(mn, (unsigned)__shfl_xor((int)mn, off));
  }
  __shared__ unsigned smx[4], smn[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    smx[w] = mx;
    smn[w] = mn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {
      mx = max(mx, smx[i]);
      mn = min(mn, smn[i]);
    }
    atomicMax(&mm[0], mx);
    atomicMin(&mm[1], mn);
  }
}

// Presets mm = {0, ~0} on the stream (a kernel, not a host copy: stream-ordered without a host
// sync, and capturable into a graph).
__global__ void minmax_init_kernel(unsigned* __restrict__ mm) {
  if (threadIdx.x == 0) {
    mm[0] = 0u;
    mm[1] = 0xffffffffu;
  }
}

static int launch_minmax(const float* x, int64_t n, int64_t stride, unsigned* mm, hipStream_t s) {
  hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(64), 0, s, mm);
  if (int rc = check_launch("minmax_init_kernel")) return rc;
  const int64_t blocks = n > 0 ? (n + 255) / 256 : 1;
  hipLaunchKernelGGL(minmax_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, x, n, stride, mm);
  return check_launch("minmax_kernel");
}

__device__ __forceinline__ uint8_t to_u8(float v) {      // np.clip(v, 0, 255).astype(np.uint8)
  return (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);
}

// run.py:248  depth_norm = (d - min) / (max - min + 1e-6)   (float32 array, Python 1e-6 as float32)
__global__ void __launch_bounds__(256) depth_norm_kernel(const float* __restrict__ d, int64_t n,
                                                          const unsigned* __restrict__ mm, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float mx = ord2f(mm[0]), mn = ord2f(mm[1]);
  out[i] = (d[i] - mn) / ((mx - mn) + 1e-6f);
}

// a**3.0 rounded once to float: a*a is exact in double (48 significant bits), the second product
// rounds to double and then to float.  numpy's float32 power is its SIMD pow (SVML on AVX-512
// hosts, libm elsewhere), within 1 ulp of this and host-dependent; oracle/post_oracle.py's fog
// takes either cube (tests/test_post_effects.py compares both).
__device__ __forceinline__ float cube_rn(float a) {
  const double d = (double)a;
  return (float)((d * d) * d);
}

// post_processor.py:451-493 (Fog): fog colour pure white, fog_start from the parameters.
//   dn = depth (/ max when max > 1); a = clip(max(dn - start, 0) / (1 - start), 0, 1)**3 * 0.3
//   out = clip(img * a + 255 * (1 - a), 0, 255) as uint8; without depth: img * 0.05 + 255 * 0.95.
// start_f / denom_f are float32(fog_start) and float32(1.0 - fog_start) (numpy's weak scalars).
__device__ __forceinline__ void fog_pixel(const uint8_t (&img)[3], float dn, float dmax, float start_f, float denom_f,
                                          uint8_t* __restrict__ out) {
  if (dmax > 1.0f) dn = dn / dmax;
  float a = fmaxf(dn - start_f, 0.0f) / denom_f;
  a = fminf(fmaxf(a, 0.0f), 1.0f);
  a = cube_rn(a);
  a = a * 0.3f;
  const float keep = 1.0f - a;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = to_u8((float)img[c] * a + 255.0f * keep);
}

__global__ void __launch_bounds__(256) fog_kernel(const uint8_t* __restrict__ img, const float* __restrict__ depth,
                                                   int64_t dstride, int64_t P, const unsigned* __restrict__ mm,
                                                   float start_f, float denom_f, uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  if (!depth) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * p + c] = to_u8((float)img[3 * p + c] * 0.05f + 255.0f * 0.95f);
    return;
  }
  const uint8_t px[3] = {img[3 * p], img[3 * p + 1], img[3 * p + 2]};
  fog_pixel(px, depth[p * dstride], ord2f(mm[0]), start_f, denom_f, out + 3 * p);
}

// The CLI's Fog frame (run.py:233 -> :248 -> post_processor.py:451-493) from the render outputs in
// one pass after the depth reduction:
//   img = uint8(rgb * 255) (truncation), dn = (d - min) / (max - min + 1e-6), Fog(img, dn).
// Fog's own maximum of dn is the normalised maximum, exactly: the normalisation is two correctly
// rounded, non-decreasing operations, so max(norm(d)) = norm(max d); no second reduction.
__global__ void __launch_bounds__(256) frame_fog_kernel(const float* __restrict__ rgb, const float* __restrict__ depth,
                                                         int64_t P, const unsigned* __restrict__ mm, float start_f,
                                                         float denom_f, uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float mx = ord2f(mm[0]), mn = ord2f(mm[1]);
  const float range = (mx - mn) + 1e-6f;
  uint8_t px[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) px[c] = (uint8_t)(int)(rgb[3 * p + c] * 255.0f);   // rgb in [0, 1]
  fog_pixel(px, (depth[p] - mn) / range, (mx - mn) / range, start_f, denom_f, out + 3 * p);
}

// ---------------------------------------------------------------------------------- Toon
// cv2 BORDER_DEFAULT = BORDER_REFLECT_101: -1 -> 1, n -> n-2.
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

constexpr int kBilRadius = 4;                       // bilateralFilter(d=9): radius d/2
constexpr int kBilNumBins = 1 << 12;                // OpenCV's kExpNumBinsPerChannel (one channel)

// Normalised depth (post_processor.py:76-78): d / max when max > 1.
__device__ __forceinline__ float toon_dn(const float* depth, int64_t i, int64_t dstride, float dmax) {
  const float v = depth[i * dstride];
  return dmax > 1.0f ? v / dmax : v;
}

// cv2.bilateralFilter(depth_norm, 9, 75, 75) on float32 (OpenCV 4 bilateralFilter_32f): value range
// [minv, maxv] of the image, a 4096-bin colour LUT exp(-0.5 (i/scale)^2 / sigma_c^2) linearly
// interpolated, spatial weights exp(-0.5 r^2 / sigma_s^2) on the radius-4 disk without the centre,
// which enters with weight 1; reflect-101 borders.  A constant image is copied.
__global__ void __launch_bounds__(256) bilateral_kernel(const float* __restrict__ depth, int64_t dstride, int H, int W,
                                                         const unsigned* __restrict__ mm, float* __restrict__ out) {
  __shared__ float lut[kBilNumBins + 2];
  __shared__ float sw[(2 * kBilRadius + 1) * (2 * kBilRadius + 1)];
  __shared__ int sdy[(2 * kBilRadius + 1) * (2 * kBilRadius + 1)], sdx[(2 * kBilRadius + 1) * (2 * kBilRadius + 1)];
  __shared__ int nk;
  const float dmax_raw = ord2f(mm[0]), dmin_raw = ord2f(mm[1]);
  const float maxv = dmax_raw > 1.0f ? dmax_raw / dmax_raw : dmax_raw;
  const float minv = dmax_raw > 1.0f ? dmin_raw / dmax_raw : dmin_raw;
  const double gcc = -0.5 / (75.0 * 75.0), gsc = -0.5 / (75.0 * 75.0);
  const float len = (float)((double)maxv - (double)minv);    // minMaxLoc's doubles, then float
  const float scale_index = (float)kBilNumBins / len;
  for (int i = threadIdx.x; i < kBilNumBins + 2; i += blockDim.x) {
    const double v = i / scale_index;
    lut[i] = (float)exp(v * v * gcc);   // stays > 0 over the table at sigma 75 (no zero tail)
  }
  if (threadIdx.x == 0) {
    int k = 0;
    for (int i = -kBilRadius; i <= kBilRadius; ++i)
      for (int j = -kBilRadius; j <= kBilRadius; ++j) {
        const double r = sqrt((double)i * i + (double)j * j);
        if (r > kBilRadius || (i == 0 && j == 0)) continue;
        sw[k] = (float)exp(r * r * gsc);
        sdy[k] = i;
        sdx[k] = j;
        ++k;
      }
    nk = k;
  }
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const float val0 = toon_dn(depth, p, dstride, dmax_raw);
  if (fabsf(maxv - minv) < FLT_EPSILON) {
    out[p] = val0;
    return;
  }
  float sum = 0.0f, wsum = 0.0f;
  for (int k = 0; k < nk; ++k) {
    const int yy = reflect101(y + sdy[k], H), xx = reflect101(x + sdx[k], W);
    const float val = toon_dn(depth, (int64_t)yy * W + xx, dstride, dmax_raw);
    float alpha = fabsf(val - val0) * scale_index;
    const int idx = (int)floorf(alpha);
    alpha -= (float)idx;
    const float w = sw[k] * (lut[idx] + alpha * (lut[idx + 1] - lut[idx]));
    wsum += w;
    sum += val * w;
  }
  out[p] = (sum + val0) / (wsum + 1.0f);
}

// cv2.Sobel(f, CV_32F, 1, 0, 3) and (0, 1): separable [-1 0 1] x [1 2 1] with reflect-101
// borders (row pass first: r = s[x+1] - s[x-1], column pass: 2 r[y] + (r[y-1] + r[y+1])),
// magnitude sqrt(gx^2 + gy^2) (post_processor.py:84-86); max into mm[0].
__device__ __forceinline__ float at101(const float* f, int y, int x, int H, int W) {
  return f[(int64_t)reflect101(y, H) * W + reflect101(x, W)];
}
__global__ void __launch_bounds__(256) sobel_kernel(const float* __restrict__ f, int H, int W, float* __restrict__ mag) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  // gx: row pass [-1 0 1] on rows y-1, y, y+1, column pass [1 2 1]
  float rx[3];
#pragma unroll
  for (int k = -1; k <= 1; ++k) rx[k + 1] = at101(f, y + k, x + 1, H, W) - at101(f, y + k, x - 1, H, W);
  const float gx = rx[1] * 2.0f + (rx[0] + rx[2]);
  // gy: row pass [1 2 1] on rows y-1, y+1, column pass [-1 0 1]
  float hy[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int yy = y - 1 + 2 * k;
    hy[k] = at101(f, yy, x, H, W) * 2.0f + (at101(f, yy, x - 1, H, W) + at101(f, yy, x + 1, H, W));
  }
  const float gy = hy[1] - hy[0];
  mag[p] = sqrtf(gx * gx + gy * gy);
}

// No-depth fallback (post_processor.py:105-111): cv2.cvtColor(RGB2GRAY) in 14-bit fixed point,
// |cv2.Laplacian(gray, CV_32F)| (ksize 1: [0 1 0; 1 -4 1; 0 1 0], reflect-101).
__device__ __forceinline__ float gray_at(const uint8_t* img, int y, int x, int H, int W) {
  const int64_t q = (int64_t)reflect101(y, H) * W + reflect101(x, W);
  const int v = (img[3 * q] * 4899 + img[3 * q + 1] * 9617 + img[3 * q + 2] * 1868 + (1 << 13)) >> 14;
  return (float)v;
}
__global__ void __launch_bounds__(256) laplacian_kernel(const uint8_t* __restrict__ img, int H, int W,
                                                         float* __restrict__ mag) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const float c = gray_at(img, y, x, H, W);
  const float l = gray_at(img, y - 1, x, H, W) + gray_at(img, y, x - 1, H, W) + gray_at(img, y, x + 1, H, W) +
                  gray_at(img, y + 1, x, H, W) - 4.0f * c;
  mag[p] = fabsf(l);
}

// Quantised colours with the edge mask (post_processor.py:71-72, :88-100 / :108-115):
//   q = floor(img / 255 * levels) / levels * 255;  e = mag / max(mag) > thr (max > 0), dilated 3x3
//   for depth edges (cv2.dilate, border ignored);  out = clip(q * (1 - strength * e)) as uint8.
__global__ void __launch_bounds__(256) toon_combine_kernel(const uint8_t* __restrict__ img, const float* __restrict__ mag,
                                                            const unsigned* __restrict__ mm, int H, int W, float levels,
                                                            float strength, float thr, int dilate,
                                                            uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const float gmax = ord2f(mm[0]);
  auto edge_at = [&](int yy, int xx) {
    float g = mag[(int64_t)yy * W + xx];
    if (gmax > 0.0f) g = g / gmax;
    return g > thr;
  };
  bool e = false;
  if (dilate) {
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) e = e || edge_at(yy, xx);
      }
  } else {
    e = edge_at(y, x);
  }
  const float ef = e ? 1.0f : 0.0f;
  const float k = 1.0f - strength * ef;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = (float)img[3 * p + c];
    const float q = floorf(v / 255.0f * levels) / levels * 255.0f;
    out[3 * p + c] = to_u8(q * k);
  }
}


// ============================================================== the seven further effects
// Vignette (:161-186), Cross Processing (:271-298), Film Grain (:214-224), Hologram (:373-449),
// Posterize (:300-318), Bloom (:146-159), Pencil Sketch (:226-269).  See the file header for what
// is pinned to the reference and what is restated.

__device__ __forceinline__ uint8_t to_u8d(double v) {     // np.clip(v, 0, 255).astype(np.uint8), float64
  return (uint8_t)(int)fmin(fmax(v, 0.0), 255.0);
}
__device__ __forceinline__ int gray_px(const uint8_t* px) {   // cvtColor(RGB2GRAY), 14-bit fixed point
  return (px[0] * 4899 + px[1] * 9617 + px[2] * 1868 + (1 << 13)) >> 14;
}
// (x - W//2)**2 + (y - H//2)**2 of np.ogrid (int64)
__device__ __forceinline__ int64_t radial2(int y, int x, int H, int W) {
  const int64_t dx = x - W / 2, dy = y - H / 2;
  return dx * dx + dy * dy;
}

// Vignette: dist = sqrt(r2) / sqrt(cx^2 + cy^2), v = clip(1 - dist * strength, 0, 1), all float64
// (np.sqrt of an int64 array); float32(img) * v is a float64 product stored into a float32 array.
__global__ void __launch_bounds__(256) vignette_kernel(const uint8_t* __restrict__ img, int H, int W, double strength,
                                                        uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const int64_t cx = W / 2, cy = H / 2;
  const double dist = sqrt((double)radial2(y, x, H, W)) / sqrt((double)(cx * cx + cy * cy));
  const double v = fmin(fmax(1.0 - dist * strength, 0.0), 1.0);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * p + c] = to_u8((float)((double)(float)img[3 * p + c] * v));
}

// Cross Processing: float32 channel gains 1.1 / 1.3 / 0.8 clipped to [0, 1], contrast
// (f - 0.5) * 1.4 + 0.5, uint8 by truncation, then the float64 mask
// clip(1.2 - r2 / (W/2)^2 * 0.4, 0, 1) and a second truncation.
__global__ void __launch_bounds__(256) cross_kernel(const uint8_t* __restrict__ img, int H, int W,
                                                     uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const double half = (double)W / 2.0;
  const double m = (double)radial2(y, x, H, W) / (half * half);
  const double mask = fmin(fmax(1.2 - m * 0.4, 0.0), 1.0);
  const float gain[3] = {1.1f, 1.3f, 0.8f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float f = (float)img[3 * p + c] / 255.0f;
    f = fminf(fmaxf(f * gain[c], 0.0f), 1.0f);
    f = (f - 0.5f) * 1.4f + 0.5f;
    const uint8_t r = to_u8(f * 255.0f);
    out[3 * p + c] = (uint8_t)(int)((double)(float)r * mask);
  }
}

// Film Grain: img + grain * amount in float32 (grain: float32 draws of N(0, 50), one per value).
__global__ void __launch_bounds__(256) grain_kernel(const uint8_t* __restrict__ img, const float* __restrict__ grain,
                                                     int64_t n, float amount, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = to_u8((float)img[i] + grain[i] * amount);
}

// Posterize: float32 quantisation (as Toon's); edges where |Laplacian(gray)| > 20 (integers, exact);
// there 255 * 0.3 + float64(q * 0.7f) in float64, elsewhere q.
__global__ void __launch_bounds__(256) posterize_kernel(const uint8_t* __restrict__ img, int H, int W, float levels,
                                                         uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  auto g = [&](int yy, int xx) { return gray_px(img + 3 * ((int64_t)reflect101(yy, H) * W + reflect101(xx, W))); };
  const int lap = g(y - 1, x) + g(y, x - 1) + g(y, x + 1) + g(y + 1, x) - 4 * g(y, x);
  const bool edge = (lap < 0 ? -lap : lap) > 20;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float q = floorf((float)img[3 * p + c] / 255.0f * levels) / levels * 255.0f;
    out[3 * p + c] = to_u8d(edge ? 255.0 * 0.3 + (double)(q * 0.7f) : (double)q);
  }
}

// ------------------------------------------------------------------ separable Gaussian blur
// cv2.GaussianBlur(src, (k, k), 0) on uint8, 1 or 3 interleaved channels, odd k <= 63, restated
// (cv2 is not installed: parity unpinned; cv2's 8-bit path uses fixed-point coefficients and may
// differ by a count).  Coefficients: nerf_gaussian_blur's comment below.  Horizontal pass into a
// float32 plane, vertical pass from it; each accumulates the taps in order i = 0..k-1 with one
// multiply and one add rounding per tap; reflect-101 borders reflected repeatedly; the vertical
// pass rounds half to even, saturates and stores uint8.  Both passes stage their inputs in an LDS
// tile with the halo, so each input is read from memory once per tile, not once per tap.
constexpr int kBlurMaxK = 63;
struct BlurTaps {
  int k;
  float w[kBlurMaxK];
};
constexpr int kBlurTW = 256;     // horizontal pass: pixels of one row per block
constexpr int kBlurCols = 64;    // vertical pass: 64 columns x 32 rows per block
constexpr int kBlurRows = 32;
enum { kSrcU8 = 0, kSrcInvGray = 1 };   // the pass reads the image, or 255 - gray(RGB) (Pencil Sketch)

template <int C, int SRC>
__global__ void __launch_bounds__(256) blur_h_kernel(const uint8_t* __restrict__ src, int H, int W, BlurTaps taps,
                                                      float* __restrict__ mid) {
  __shared__ float tile[(kBlurTW + kBlurMaxK - 1) * C];
  __shared__ float sw[kBlurMaxK];
  const int k = taps.k, r = k >> 1;
  const unsigned nbx = (unsigned)((W + kBlurTW - 1) / kBlurTW);
  const int y = (int)(blockIdx.x / nbx), x0 = (int)(blockIdx.x % nbx) * kBlurTW;
  const int tw = min(kBlurTW, W - x0);
  if ((int)threadIdx.x < k) sw[threadIdx.x] = taps.w[threadIdx.x];
  const uint8_t* row = src + (int64_t)y * W * (SRC == kSrcInvGray ? 3 : C);
  for (int j = threadIdx.x; j < tw + 2 * r; j += 256) {
    const int xx = reflect101(x0 - r + j, W);
    if (SRC == kSrcInvGray) {
      tile[j] = (float)(255 - gray_px(row + 3 * xx));
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) tile[j * C + c] = (float)row[xx * C + c];
    }
  }
  __syncthreads();
  float* dst = mid + ((int64_t)y * W + x0) * C;
  for (int e = threadIdx.x; e < tw * C; e += 256) {
    float acc = 0.0f;
    for (int i = 0; i < k; ++i) acc = acc + sw[i] * tile[e + i * C];
    dst[e] = acc;
  }
}

// What the vertical pass does with a blurred value b (uint8):
//   kEpiStore   out = b
//   kEpiBloom   cv2.addWeighted(img, 1, blur, beta, 0) restated: img + b * beta in float32 (separate
//               multiply and add), rounded half to even, saturated
//   kEpiSketch  Pencil Sketch from `b` = blur(255 - gray): sketch = cv2.divide(gray, 255 - b, 256)
//               (0 where the divisor is 0, else rint(256 gray / divisor) saturated), the depth mask
//               1 - clip((dn - thr) * 5, 0, 1) (float32; 1 without depth), then per channel
//               float32(((1 - s) img + s sketch) * mask) [float64] + img * (1 - mask) [float32].
enum { kEpiStore = 0, kEpiBloom = 1, kEpiSketch = 2 };
struct BlurEpi {
  int mode;
  const uint8_t* img;
  float beta;
  const float* depth;
  const unsigned* mm;
  const float* thr;
  double s, oms;
};

__global__ void __launch_bounds__(256) blur_v_kernel(const float* __restrict__ mid, int H, int64_t N, BlurTaps taps,
                                                      BlurEpi epi, uint8_t* __restrict__ out) {
  __shared__ float tile[kBlurRows + kBlurMaxK - 1][kBlurCols];
  __shared__ float sw[kBlurMaxK];
  const int k = taps.k, r = k >> 1;
  const unsigned nbx = (unsigned)((N + kBlurCols - 1) / kBlurCols);
  const int64_t c0 = (int64_t)(blockIdx.x % nbx) * kBlurCols;
  const int y0 = (int)(blockIdx.x / nbx) * kBlurRows;
  const int cw = (int)imin64(kBlurCols, N - c0), th = min(kBlurRows, H - y0);
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  if ((int)threadIdx.x < k) sw[threadIdx.x] = taps.w[threadIdx.x];
  if (lx < cw)
    for (int j = ly; j < th + 2 * r; j += 4) tile[j][lx] = mid[(int64_t)reflect101(y0 - r + j, H) * N + c0 + lx];
  __syncthreads();
  if (lx >= cw) return;
  for (int yy = ly; yy < th; yy += 4) {
    float acc = 0.0f;
    for (int i = 0; i < k; ++i) acc = acc + sw[i] * tile[yy + i][lx];
    const int b = (int)fminf(fmaxf(rintf(acc), 0.0f), 255.0f);
    const int64_t e = (int64_t)(y0 + yy) * N + c0 + lx;
    if (epi.mode == kEpiStore) {
      out[e] = (uint8_t)b;
    } else if (epi.mode == kEpiBloom) {
      out[e] = (uint8_t)(int)fminf(fmaxf(rintf((float)epi.img[e] + (float)b * epi.beta), 0.0f), 255.0f);
    } else {
      const uint8_t* px = epi.img + 3 * e;
      const int g = gray_px(px), div = 255 - b;
      const double sk = div == 0 ? 0.0 : fmin(rint((double)(256 * g) / (double)div), 255.0);
      float m = 1.0f;
      if (epi.depth) {
        const float dmax = ord2f(epi.mm[0]);
        float dn = epi.depth[e];
        if (dmax > 1.0f) dn = dn / dmax;
        m = 1.0f - fminf(fmaxf((dn - epi.thr[0]) * 5.0f, 0.0f), 1.0f);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float v = (float)((epi.oms * (double)px[c] + epi.s * sk) * (double)m);
        v = v + (float)px[c] * (1.0f - m);
        out[3 * e + c] = to_u8(v);
      }
    }
  }
}

static int launch_blur(const uint8_t* src, int H, int W, int C, int src_mode, const BlurTaps& taps, float* mid,
                       const BlurEpi& epi, uint8_t* out, hipStream_t s) {
  const unsigned hb = (unsigned)((W + kBlurTW - 1) / kBlurTW) * (unsigned)H;
  if (src_mode == kSrcInvGray)
    hipLaunchKernelGGL((blur_h_kernel<1, kSrcInvGray>), dim3(hb), dim3(256), 0, s, src, H, W, taps, mid);
  else if (C == 1)
    hipLaunchKernelGGL((blur_h_kernel<1, kSrcU8>), dim3(hb), dim3(256), 0, s, src, H, W, taps, mid);
  else
    hipLaunchKernelGGL((blur_h_kernel<3, kSrcU8>), dim3(hb), dim3(256), 0, s, src, H, W, taps, mid);
  if (int rc = check_launch("blur_h_kernel")) return rc;
  const int64_t N = (int64_t)W * C;
  const unsigned vb = (unsigned)((N + kBlurCols - 1) / kBlurCols) * (unsigned)((H + kBlurRows - 1) / kBlurRows);
  hipLaunchKernelGGL(blur_v_kernel, dim3(vb), dim3(256), 0, s, mid, H, N, taps, epi, out);
  return check_launch("blur_v_kernel");
}

// ------------------------------------------------------------------------ exact percentile
// Order statistics k0 <= k1 of x[i*stride], i < n, by radix select on the f2ord keys: four passes
// of 8 bits from the top; each pass counts, per target, the digit of every key that matches the
// target's prefix so far (LDS-private 256-bin histograms merged by integer atomics: exact and the
// same in any order), then one small block walks the bins to the digit that holds the rank.
struct SelectState {
  unsigned hist[2][256];
  unsigned prefix[2];
  unsigned rank[2];
  float value;
};

__global__ void select_init_kernel(SelectState* __restrict__ st, unsigned k0, unsigned k1) {
  for (int i = threadIdx.x; i < 512; i += blockDim.x) (&st->hist[0][0])[i] = 0u;
  if (threadIdx.x < 2) {
    st->prefix[threadIdx.x] = 0u;
    st->rank[threadIdx.x] = threadIdx.x ? k1 : k0;
  }
}

__global__ void __launch_bounds__(256) select_hist_kernel(const float* __restrict__ x, int64_t n, int64_t stride,
                                                           SelectState* __restrict__ st, int pass) {
  __shared__ unsigned h[2][256];
  h[0][threadIdx.x] = 0u;
  h[1][threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned himask = pass ? 0xffffffffu << (shift + 8) : 0u;
  const unsigned p0 = st->prefix[0], p1 = st->prefix[1];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned key = f2ord(x[i * stride]);
    const unsigned d = (key >> shift) & 255u;
    if ((key & himask) == p0) atomicAdd(&h[0][d], 1u);
    if ((key & himask) == p1) atomicAdd(&h[1][d], 1u);
  }
  __syncthreads();
  if (h[0][threadIdx.x]) atomicAdd(&st->hist[0][threadIdx.x], h[0][threadIdx.x]);
  if (h[1][threadIdx.x]) atomicAdd(&st->hist[1][threadIdx.x], h[1][threadIdx.x]);
}

__global__ void select_scan_kernel(SelectState* __restrict__ st, int pass) {
  if (threadIdx.x < 2) {
    const int t = threadIdx.x;
    const unsigned rank = st->rank[t];
    unsigned cum = 0u;
    int d = 0;
    for (; d < 255; ++d) {
      const unsigned c = st->hist[t][d];
      if (rank < cum + c) break;
      cum += c;
    }
    st->prefix[t] |= (unsigned)d << (24 - 8 * pass);
    st->rank[t] = rank - cum;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 512; i += blockDim.x) (&st->hist[0][0])[i] = 0u;
}

// numpy's "linear" interpolation in float32 between a = x_(k0) and b = x_(k1): a + (b - a) t, or
// b - (b - a)(1 - t) where t >= 0.5 (np.percentile's _lerp).  With mm, the values are first divided
// by the maximum when it exceeds 1 (the effects' depth normalisation: monotone, so the order
// statistics of the normalised plane are the normalised order statistics).
__global__ void select_finish_kernel(SelectState* __restrict__ st, const unsigned* __restrict__ mm, float t,
                                     float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  float a = ord2f(st->prefix[0]), b = ord2f(st->prefix[1]);
  if (mm) {
    const float mx = ord2f(mm[0]);
    if (mx > 1.0f) {
      a = a / mx;
      b = b / mx;
    }
  }
  const float d = b - a;
  const float v = t >= 0.5f ? b - d * (1.0f - t) : a + d * t;
  st->value = v;
  if (out) out[0] = v;
}

// np.percentile's float32 index arithmetic (numpy 2: the quantile q / 100, the virtual index
// (n - 1) * quantile and its fraction are all float32 for a float32 array).
static void percentile_plan(int64_t n, double q, int64_t* k0, int64_t* k1, float* t) {
  const float quant = (float)q / 100.0f;
  const float last = (float)(n - 1);
  const float v = last * quant;
  if (v >= last) {
    *k0 = *k1 = n - 1;
    *t = 0.0f;
    return;
  }
  const float lo = floorf(v);
  *k0 = imin64((int64_t)lo, n - 1);
  *k1 = imin64(*k0 + 1, n - 1);
  *t = v - lo;
}

static int launch_percentile(const float* x, int64_t n, int64_t stride, double q, SelectState* st, const unsigned* mm,
                             float* out, hipStream_t s) {
  int64_t k0, k1;
  float t;
  percentile_plan(n, q, &k0, &k1, &t);
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(256), 0, s, st, (unsigned)k0, (unsigned)k1);
  if (int rc = check_launch("select_init_kernel")) return rc;
  const int64_t blocks = (n + 255) / 256;
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(select_hist_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, x, n,
                       stride, st, pass);
    if (int rc = check_launch("select_hist_kernel")) return rc;
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(64), 0, s, st, pass);
    if (int rc = check_launch("select_scan_kernel")) return rc;
  }
  hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(64), 0, s, st, mm, t, out);
  return check_launch("select_finish_kernel");
}

// -------------------------------------------------------------------------------- Hologram
// Scanline factor of each row (:385-393): line i darkens rows [int(i lh), int(min((i + 0.7) lh, H)))
// by 0.85, lh = H / lines in float64; a row covered by several lines (H < lines) is multiplied
// that many times, sequentially, in float32.
__global__ void __launch_bounds__(256) holo_rows_kernel(int H, int lines, float* __restrict__ fac) {
  const int y = blockIdx.x * blockDim.x + threadIdx.x;
  if (y >= H) return;
  const double lh = (double)H / (double)lines;
  float f = 1.0f;
  for (int i = 0; i < lines; ++i) {
    const int ys = (int)((double)i * lh);
    const double e = ((double)i + 0.7) * lh;
    const int ye = (int)(e < (double)H ? e : (double)H);
    if (y >= ys && y < ye) f = f * 0.85f;
  }
  fac[y] = f;
}

__global__ void __launch_bounds__(256) plane_dn_kernel(const float* __restrict__ depth, int64_t dstride, int64_t P,
                                                        const unsigned* __restrict__ mm, float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < P) out[p] = toon_dn(depth, p, dstride, ord2f(mm[0]));
}

// Column spans brightened by 1.5 (:443-447): [pos, min(pos + width, W)), three of them, applied in
// order (overlaps multiply twice); by value, or read from device memory as int64 (pos, width) pairs.
struct HoloSpans {
  int pos[3], width[3];
};

// cyan tint (img / 255 times 0.8, 1.0, 0.2), scanlines, + edge glow (Sobel magnitude of the
// normalised depth over its max, times 0.1, 0.6, 0.3) + noise, spans, * 255; float32 throughout.
__global__ void __launch_bounds__(256) holo_kernel(const uint8_t* __restrict__ img, const float* __restrict__ mag,
                                                    const unsigned* __restrict__ mm, const float* __restrict__ rowfac,
                                                    const float* __restrict__ noise, int H, int W, HoloSpans spans,
                                                    const int64_t* __restrict__ spans_dev, uint8_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p % W);
  float e = 0.0f;
  if (mag) {
    const float gmax = ord2f(mm[0]);
    e = mag[p];
    if (gmax > 0.0f) e = e / gmax;
  }
  float boost = 1.0f;   // 1.5^j, exact
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int64_t x0 = spans_dev ? spans_dev[2 * j] : spans.pos[j];
    const int64_t x1 = imin64(x0 + (spans_dev ? spans_dev[2 * j + 1] : spans.width[j]), W);
    if (x >= x0 && x < x1) boost = boost * 1.5f;
  }
  const float tint[3] = {0.8f, 1.0f, 0.2f}, glow[3] = {0.1f, 0.6f, 0.3f};
  const float rf = rowfac[y];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float h = (float)img[3 * p + c] / 255.0f * tint[c] * rf;
    h = (h + (mag ? e * glow[c] : 0.0f)) + noise[3 * p + c];
    // h * 1.5 per covering span: multiplying by 1.5 up to three times in sequence
    if (boost > 1.0f) h = h * 1.5f;
    if (boost > 2.0f) h = h * 1.5f;
    if (boost > 3.0f) h = h * 1.5f;
    out[3 * p + c] = to_u8(h * 255.0f);
  }
}

}  // namespace nerf

using namespace nerf;

#define EREQUIRE(cond, ...)                                          \
  do {                                                               \
    if (!(cond)) return set_error(NERF_ERR_BAD_ARG, __VA_ARGS__);    \
  } while (0)

extern "C" {

// Workspace: [0, 256) the reductions' max/min; three float planes (Toon uses two; the blur's
// intermediate of a 3-channel image is three); kSelectBytes for the percentile's state; H floats
// for Hologram's row factors.
constexpr size_t kSelectBytes = 4096;
static_assert(sizeof(SelectState) <= kSelectBytes, "percentile state");
static size_t ws_plane(int H, int W) { return ((size_t)H * W * sizeof(float) + 255) & ~(size_t)255; }
static size_t ws_select_off(int H, int W) { return 256 + 3 * ws_plane(H, W); }
static size_t ws_rows_off(int H, int W) { return ws_select_off(H, W) + kSelectBytes; }

size_t nerf_effect_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return ws_rows_off(H, W) + (((size_t)H * sizeof(float) + 255) & ~(size_t)255);
}

int nerf_depth_normalize(const float* depth, int64_t n, float* out, void* workspace, size_t ws_bytes,
                         nerf_stream_t stream) {
  EREQUIRE(n >= 0, "nerf_depth_normalize: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  EREQUIRE(depth && out && workspace && ws_bytes >= 256, "nerf_depth_normalize: null pointer or workspace < 256 B");
  hipStream_t s = (hipStream_t)stream;
  unsigned* mm = (unsigned*)workspace;
  if (int rc = launch_minmax(depth, n, 1, mm, s)) return rc;
  hipLaunchKernelGGL(depth_norm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, depth, n, mm, out);
  return check_launch("depth_norm_kernel");
}

int nerf_effect_fog(const uint8_t* image, const float* depth, int64_t depth_stride, int H, int W, double fog_start,
                    uint8_t* out, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0 && depth_stride >= 1, "nerf_effect_fog: H=%d W=%d stride=%lld", H, W,
           (long long)depth_stride);
  EREQUIRE(image && out && workspace && ws_bytes >= nerf_effect_workspace_bytes(H, W),
           "nerf_effect_fog: null pointer or workspace too small");
  EREQUIRE(fog_start < 1.0, "nerf_effect_fog: fog_start=%g must be < 1", fog_start);
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = (int64_t)H * W;
  unsigned* mm = (unsigned*)workspace;
  if (depth)
    if (int rc = launch_minmax(depth, P, depth_stride, mm, s)) return rc;
  hipLaunchKernelGGL(fog_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, image, depth, depth_stride, P, mm,
                     (float)fog_start, (float)(1.0 - fog_start), out);
  return check_launch("fog_kernel");
}

int nerf_frame_fog(const float* rgb, const float* depth, int H, int W, double fog_start, uint8_t* out,
                   void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0, "nerf_frame_fog: H=%d W=%d", H, W);
  EREQUIRE(rgb && depth && out && workspace && ws_bytes >= 256, "nerf_frame_fog: null pointer or workspace < 256 B");
  EREQUIRE(fog_start < 1.0, "nerf_frame_fog: fog_start=%g must be < 1", fog_start);
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = (int64_t)H * W;
  unsigned* mm = (unsigned*)workspace;
  if (int rc = launch_minmax(depth, P, 1, mm, s)) return rc;
  hipLaunchKernelGGL(frame_fog_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, rgb, depth, P, mm,
                     (float)fog_start, (float)(1.0 - fog_start), out);
  return check_launch("frame_fog_kernel");
}

int nerf_effect_toon(const uint8_t* image, const float* depth, int64_t depth_stride, int H, int W, double levels,
                     double edge_strength, uint8_t* out, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0 && depth_stride >= 1 && levels > 0.0, "nerf_effect_toon: H=%d W=%d stride=%lld levels=%g",
           H, W, (long long)depth_stride, levels);
  EREQUIRE(image && out && workspace && ws_bytes >= nerf_effect_workspace_bytes(H, W),
           "nerf_effect_toon: null pointer or workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = (int64_t)H * W;
  const unsigned blocks = (unsigned)((P + 255) / 256);
  unsigned* mm = (unsigned*)workspace;
  const size_t plane = ((size_t)P * sizeof(float) + 255) & ~(size_t)255;
  float* filt = (float*)((char*)workspace + 256);
  float* mag = (float*)((char*)workspace + 256 + plane);
  int rc;
  if (depth) {
    if ((rc = launch_minmax(depth, P, depth_stride, mm, s))) return rc;
    hipLaunchKernelGGL(bilateral_kernel, dim3(blocks), dim3(256), 0, s, depth, depth_stride, H, W, mm, filt);
    if ((rc = check_launch("bilateral_kernel"))) return rc;
    hipLaunchKernelGGL(sobel_kernel, dim3(blocks), dim3(256), 0, s, filt, H, W, mag);
    if ((rc = check_launch("sobel_kernel"))) return rc;
  } else {
    hipLaunchKernelGGL(laplacian_kernel, dim3(blocks), dim3(256), 0, s, image, H, W, mag);
    if ((rc = check_launch("laplacian_kernel"))) return rc;
  }
  if ((rc = launch_minmax(mag, P, 1, mm, s))) return rc;
  hipLaunchKernelGGL(toon_combine_kernel, dim3(blocks), dim3(256), 0, s, image, mag, mm, H, W, (float)levels,
                     (float)edge_strength, depth ? 0.05f : 0.1f, depth ? 1 : 0, out);
  return check_launch("toon_combine_kernel");
}

// cv2.getGaussianKernel(k, 0) as float32, on the host: OpenCV's fixed tables for k = 1, 3, 5, 7;
// otherwise sigma = 0.3 ((k - 1) 0.5 - 1) + 0.8 and w_i = exp(-(i - (k-1)/2)^2 / (2 sigma^2)), in
// double, divided by their double sum (added in order), then rounded to float32.
static bool gaussian_taps(int k, BlurTaps* taps) {
  if (k < 1 || k > kBlurMaxK || k % 2 == 0) return false;
  static const float small[4][7] = {{1.f},
                                    {.25f, .5f, .25f},
                                    {.0625f, .25f, .375f, .25f, .0625f},
                                    {.03125f, .109375f, .21875f, .28125f, .21875f, .109375f, .03125f}};
  taps->k = k;
  for (int i = 0; i < kBlurMaxK; ++i) taps->w[i] = 0.0f;
  if (k <= 7) {
    for (int i = 0; i < k; ++i) taps->w[i] = small[k / 2][i];
    return true;
  }
  const double sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8;
  double w[kBlurMaxK], sum = 0.0;
  for (int i = 0; i < k; ++i) {
    const double x = i - (k - 1) * 0.5;
    w[i] = exp(-(x * x) / (2.0 * sigma * sigma));
    sum += w[i];
  }
  for (int i = 0; i < k; ++i) taps->w[i] = (float)(w[i] / sum);
  return true;
}

static bool blur_grid_fits(int H, int W) {   // block counts of both passes stay below 2^31
  return ((int64_t)(W + kBlurTW - 1) / kBlurTW) * H < (1ll << 31) &&
         (((int64_t)W * 3 + kBlurCols - 1) / kBlurCols) * ((H + kBlurRows - 1) / kBlurRows) < (1ll << 31);
}

int nerf_gaussian_blur(const uint8_t* image, int H, int W, int C, int k, uint8_t* out, void* workspace,
                       size_t ws_bytes, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0 && (C == 1 || C == 3) && blur_grid_fits(H, W), "nerf_gaussian_blur: H=%d W=%d C=%d", H, W, C);
  BlurTaps taps;
  EREQUIRE(gaussian_taps(k, &taps), "nerf_gaussian_blur: k=%d must be odd and within 1..%d", k, kBlurMaxK);
  EREQUIRE(image && out && workspace && ws_bytes >= nerf_effect_workspace_bytes(H, W),
           "nerf_gaussian_blur: null pointer or workspace too small");
  BlurEpi epi = {};
  epi.mode = kEpiStore;
  return launch_blur(image, H, W, C, kSrcU8, taps, (float*)((char*)workspace + 256), epi, out, (hipStream_t)stream);
}

int nerf_effect_bloom(const uint8_t* image, int H, int W, int size, double strength, uint8_t* out, void* workspace,
                      size_t ws_bytes, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0 && blur_grid_fits(H, W), "nerf_effect_bloom: H=%d W=%d", H, W);
  BlurTaps taps;
  EREQUIRE(size < kBlurMaxK + 1 && gaussian_taps(size % 2 == 0 ? size + 1 : size, &taps),
           "nerf_effect_bloom: bloom size %d (odd, or the next odd number) must be within 1..%d", size, kBlurMaxK);
  EREQUIRE(image && out && workspace && ws_bytes >= nerf_effect_workspace_bytes(H, W),
           "nerf_effect_bloom: null pointer or workspace too small");
  BlurEpi epi = {};
  epi.mode = kEpiBloom;
  epi.img = image;
  epi.beta = (float)strength;
  return launch_blur(image, H, W, 3, kSrcU8, taps, (float*)((char*)workspace + 256), epi, out, (hipStream_t)stream);
}

int nerf_effect_vignette(const uint8_t* image, int H, int W, double strength, uint8_t* out, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0, "nerf_effect_vignette: H=%d W=%d", H, W);
  EREQUIRE(image && out, "nerf_effect_vignette: null pointer");
  const int64_t P = (int64_t)H * W;
  hipLaunchKernelGGL(vignette_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, image, H, W,
                     strength, out);
  return check_launch("vignette_kernel");
}

int nerf_effect_cross_processing(const uint8_t* image, int H, int W, uint8_t* out, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0, "nerf_effect_cross_processing: H=%d W=%d", H, W);
  EREQUIRE(image && out, "nerf_effect_cross_processing: null pointer");
  const int64_t P = (int64_t)H * W;
  hipLaunchKernelGGL(cross_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, image, H, W,
                     out);
  return check_launch("cross_kernel");
}

int nerf_effect_film_grain(const uint8_t* image, const float* noise, int H, int W, double amount, uint8_t* out,
                           nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0, "nerf_effect_film_grain: H=%d W=%d", H, W);
  EREQUIRE(image && noise && out, "nerf_effect_film_grain: null pointer");
  const int64_t n = (int64_t)H * W * 3;
  hipLaunchKernelGGL(grain_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, image, noise, n,
                     (float)amount, out);
  return check_launch("grain_kernel");
}

int nerf_effect_posterize(const uint8_t* image, int H, int W, double levels, uint8_t* out, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0 && levels > 0.0, "nerf_effect_posterize: H=%d W=%d levels=%g", H, W, levels);
  EREQUIRE(image && out, "nerf_effect_posterize: null pointer");
  const int64_t P = (int64_t)H * W;
  hipLaunchKernelGGL(posterize_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, image, H, W,
                     (float)levels, out);
  return check_launch("posterize_kernel");
}

int nerf_depth_percentile(const float* depth, int64_t n, int64_t stride, double q, float* out, void* workspace,
                          size_t ws_bytes, nerf_stream_t stream) {
  EREQUIRE(n >= 1 && n < (1ll << 31) && stride >= 1 && q >= 0.0 && q <= 100.0,
           "nerf_depth_percentile: n=%lld stride=%lld q=%g", (long long)n, (long long)stride, q);
  EREQUIRE(depth && out && workspace && ws_bytes >= kSelectBytes,
           "nerf_depth_percentile: null pointer or workspace < %zu B", kSelectBytes);
  return launch_percentile(depth, n, stride, q, (SelectState*)workspace, nullptr, out, (hipStream_t)stream);
}

int nerf_effect_pencil_sketch(const uint8_t* image, const float* depth, int H, int W, double strength, uint8_t* out,
                              void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && blur_grid_fits(H, W), "nerf_effect_pencil_sketch: H=%d W=%d",
           H, W);
  EREQUIRE(image && out && workspace && ws_bytes >= nerf_effect_workspace_bytes(H, W),
           "nerf_effect_pencil_sketch: null pointer or workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = (int64_t)H * W;
  unsigned* mm = (unsigned*)workspace;
  SelectState* st = (SelectState*)((char*)workspace + ws_select_off(H, W));
  if (depth) {   // 70th percentile of the normalised depth (:249-254), kept on the device
    if (int rc = launch_minmax(depth, P, 1, mm, s)) return rc;
    if (int rc = launch_percentile(depth, P, 1, 70.0, st, mm, nullptr, s)) return rc;
  }
  BlurTaps taps;
  gaussian_taps(21, &taps);
  BlurEpi epi = {};
  epi.mode = kEpiSketch;
  epi.img = image;
  epi.depth = depth;
  epi.mm = mm;
  epi.thr = &st->value;
  epi.s = strength;
  epi.oms = 1.0 - strength;
  return launch_blur(image, H, W, 1, kSrcInvGray, taps, (float*)((char*)workspace + 256), epi, out, s);
}

int nerf_effect_hologram(const uint8_t* image, const float* depth, int64_t depth_stride, int H, int W, int lines,
                         const float* noise, int x0, int w0, int x1, int w1, int x2, int w2,
                         const int64_t* spans_device, uint8_t* out, void* workspace, size_t ws_bytes,
                         nerf_stream_t stream) {
  EREQUIRE(H > 0 && W > 0 && depth_stride >= 1 && lines >= 1 && lines <= 65536,
           "nerf_effect_hologram: H=%d W=%d stride=%lld lines=%d", H, W, (long long)depth_stride, lines);
  EREQUIRE(image && noise && out && workspace && ws_bytes >= nerf_effect_workspace_bytes(H, W),
           "nerf_effect_hologram: null pointer or workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t P = (int64_t)H * W;
  const unsigned blocks = (unsigned)((P + 255) / 256);
  unsigned* mm = (unsigned*)workspace;
  float* dn = (float*)((char*)workspace + 256);
  float* mag = (float*)((char*)workspace + 256 + ws_plane(H, W));
  float* rowfac = (float*)((char*)workspace + ws_rows_off(H, W));
  int rc;
  hipLaunchKernelGGL(holo_rows_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, s, H, lines, rowfac);
  if ((rc = check_launch("holo_rows_kernel"))) return rc;
  if (depth) {   // the maximum is over every channel (:407-409), then channel 0 is used (:412-413)
    if ((rc = launch_minmax(depth, P * depth_stride, 1, mm, s))) return rc;
    hipLaunchKernelGGL(plane_dn_kernel, dim3(blocks), dim3(256), 0, s, depth, depth_stride, P, mm, dn);
    if ((rc = check_launch("plane_dn_kernel"))) return rc;
    hipLaunchKernelGGL(sobel_kernel, dim3(blocks), dim3(256), 0, s, dn, H, W, mag);
    if ((rc = check_launch("sobel_kernel"))) return rc;
    if ((rc = launch_minmax(mag, P, 1, mm, s))) return rc;
  }
  const HoloSpans spans = {{x0, x1, x2}, {w0, w1, w2}};
  hipLaunchKernelGGL(holo_kernel, dim3(blocks), dim3(256), 0, s, image, depth ? mag : nullptr, mm, rowfac, noise, H, W,
                     spans, spans_device, out);
  return check_launch("holo_kernel");
}

}  // extern "C"
