// Training path: the optimizer step and the loss value (src/train.py:87, :90-92).
//
//   adam_kernel   torch.optim.Adam's update, element for element
//   loss_kernel   the MSE from the composite backward's per-ray squared errors
#include "train_internal.h"

namespace nerf {

// ------------------------------------------------------------------------------------ Adam
// torch.optim.Adam (amsgrad=False, maximize=False, weight_decay=0) element for element:
//   m = lerp(m, g, 1-beta1);  v = v*beta2 + (1-beta2) g^2
//   p = p - step_size * m / (sqrt(v)/bc2_sqrt + eps),  step_size = lr / bc1
__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
            int64_t n, float w1, float beta2, float one_m_beta2, float bc2_sqrt, float eps, float neg_step) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  const float mi = m[i];
  // lerp as ATen's vectorised CPU kernel evaluates it (fused multiply-add), addcmul left to right
  const float m_new = w1 < 0.5f ? fmaf(w1, gi - mi, mi) : fmaf(w1 - 1.0f, gi - mi, gi);
  const float v_new = v[i] * beta2 + (one_m_beta2 * gi) * gi;
  m[i] = m_new;
  v[i] = v_new;
  const float denom = sqrtf(v_new) / bc2_sqrt + eps;
  p[i] = p[i] + neg_step * (m_new / denom);
}

int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                double eps, int64_t step, hipStream_t s) {
  if (n == 0) return NERF_OK;
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, g, m, v, n,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)sqrt(bc2), (float)eps,
                     (float)(-(lr / bc1)));
  return check_launch("adam_kernel");
}

// loss = sum(sq_err) / (3B) (F.mse_loss, reduction='mean', train.py:87), summed in double
__global__ void __launch_bounds__(256) loss_kernel(const float* __restrict__ sq_err, int64_t B, float* __restrict__ loss) {
  __shared__ double part[256];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 256) acc += (double)sq_err[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(part[0] / (3.0 * (double)B));
}

int launch_loss(const float* sq_err, int64_t B, float* loss, hipStream_t s) {
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(256), 0, s, sq_err, B, loss);
  return check_launch("loss_kernel");
}

// loss = sum(sq_err) / B: the opacity term's mean over the rays, the same reduction
// (a copy with another divisor, so that loss_kernel, which every existing step launches, stays as it is)
__global__ void __launch_bounds__(256) loss_rays_kernel(const float* __restrict__ sq_err, int64_t B,
                                                        float* __restrict__ loss) {
  __shared__ double part[256];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 256) acc += (double)sq_err[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(part[0] / (double)B);
}

int launch_loss_rays(const float* sq_err, int64_t B, float* loss, hipStream_t s) {
  hipLaunchKernelGGL(loss_rays_kernel, dim3(1), dim3(256), 0, s, sq_err, B, loss);
  return check_launch("loss_rays_kernel");
}

}  // namespace nerf
