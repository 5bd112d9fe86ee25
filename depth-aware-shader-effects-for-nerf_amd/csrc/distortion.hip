// Training path: the distortion loss of the ray weights (mip-NeRF 360's regulariser; DESIGN.md §16,
// include/nerfmi_train.h "distortion").  A penalty on the weights alone, minimal when a ray's weight sits
// in one short interval: it removes the floaters and haze that the colour loss cannot see and that
// smear the expected depth.
//
//   distortion_kernel   per ray l_r and scale * d l_r / d w_k from the forward's float weights and z,
//                       one wave per ray, double-precision prefix scans, O(T)
#include "train_internal.h"

namespace nerf {

// Per ray of T samples (z non-decreasing), sample i owns the compositor's interval, in double from the
// float z:  d_i = z_{i+1} - z_i (d_{T-1} = 1e-3f),  m_i = z_i + d_i / 2  (non-decreasing with z), and
//   l_r         = inv [ sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i ]
//   dl_r / dw_k = inv [ 2 a_k + (2/3) w_k d_k ],   a_k = sum_j w_j |m_k - m_j|
// On sorted m, with W and M the sums of w and w m before (<) and after (>) k:
//   a_k = m_k (W_<k - W_>k) - (M_<k - M_>k),  W_<k - W_>k = 2 W_<k + w_k - W  (M alike),
// and sum_i sum_j w_i w_j |m_i - m_j| = sum_k w_k a_k.
//
// Layout: composite_backward_kernel's, one wave per ray, 4 rays per 256-thread block, 64-sample chunks.
// Pass 1 sums the totals W and M (a butterfly: every lane holds the same bits).  Pass 2 forms the
// exclusive prefixes by __shfl_up scans with the chunk carries in registers, writes g_w from
// 2 prefix + own - total and sums w_k a_k + (1/3) w_k^2 d_k for the loss.  Everything is double until
// the one rounding of each output; no atomics, no traffic between waves: deterministic, and l_r is
// the same bits whether g_w is asked for or not.  T = 1: the reference's per-sample tensors are empty
// (composite_backward_kernel at N = 1), l = 0 and g = 0.  A ray of zero weights gives exact zeros (every
// term is a product with a zero weight); a descending z gives finite, otherwise unspecified values.
__global__ void __launch_bounds__(256)
distortion_kernel(const float* __restrict__ weights, const float* __restrict__ zv, int64_t B, int T, double inv,
                  double scale, float* __restrict__ loss_rays, float* __restrict__ g_w) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const int64_t base = r * (int64_t)T;
  if (T == 1) {
    if (lane == 0) {
      if (loss_rays) loss_rays[r] = 0.0f;
      if (g_w) g_w[base] = 0.0f;
    }
    return;
  }
  const int nchunk = (T + 63) / 64;
  // pass 1: the totals
  double Wt = 0.0, Mt = 0.0;
  for (int c = 0; c < nchunk; ++c) {
    const int s = c * 64 + lane;
    if (s < T) {
      const double z = (double)zv[base + s];
      const double d = (s + 1 < T) ? (double)zv[base + s + 1] - z : (double)1e-3f;
      const double w = (double)weights[base + s];
      Wt += w;
      Mt += w * (z + d * 0.5);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Wt += __shfl_xor(Wt, off);
    Mt += __shfl_xor(Mt, off);
  }
  // pass 2: exclusive prefixes, the gradient and the loss
  const double third = 1.0 / 3.0, gs = scale * inv;
  double cw = 0.0, cm = 0.0, part = 0.0;   // sums of w and w m over the chunks before this one; the loss terms
  for (int c = 0; c < nchunk; ++c) {
    const int s = c * 64 + lane;
    const bool valid = s < T;
    double w = 0.0, m = 0.0, d = 0.0;
    if (valid) {
      const double z = (double)zv[base + s];
      d = (s + 1 < T) ? (double)zv[base + s + 1] - z : (double)1e-3f;
      w = (double)weights[base + s];
      m = z + d * 0.5;
    }
    const double wm = w * m;
    double iw = w, im = wm;                // inclusive prefixes within the chunk
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double uw = __shfl_up(iw, off), um = __shfl_up(im, off);
      if (lane >= off) {
        iw += uw;
        im += um;
      }
    }
    double pw = __shfl_up(iw, 1), pm = __shfl_up(im, 1);
    if (lane == 0) pw = 0.0, pm = 0.0;
    pw += cw;
    pm += cm;
    if (valid) {
      const double a = m * (2.0 * pw + w - Wt) - (2.0 * pm + wm - Mt);
      const double own = w * d;
      if (g_w) g_w[base + s] = (float)(gs * (2.0 * a + 2.0 * third * own));
      part += w * a + third * (w * own);
    }
    cw += __shfl(iw, 63);
    cm += __shfl(im, 63);
  }
  if (loss_rays) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) loss_rays[r] = (float)(inv * part);
  }
}

int launch_distortion(const float* weights, const float* z, int64_t B, int T, double inv, double scale,
                      float* loss_rays, float* g_w, hipStream_t s) {
  if (B == 0 || (!loss_rays && !g_w)) return NERF_OK;
  hipLaunchKernelGGL(distortion_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, weights, z, B, T, inv, scale,
                     loss_rays, g_w);
  return check_launch("distortion_kernel");
}

}  // namespace nerf
