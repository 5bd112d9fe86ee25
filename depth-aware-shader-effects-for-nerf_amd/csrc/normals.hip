// Density-gradient normals (include/nerfmi_train.h "position gradient and normals"): the
// gradient of the loss with respect to the sample position from what the training kernels already
// leave behind, and a normal map built on it.
//
//   pack_input_kernel        W_0^T and W_4[:, 256:319]^T as one 64 x 512 MFMA operand (layout.h
//                            "input-gradient weights"); pack_input_host: the same buffer, bit-identical
//   position_grad_kernel     g_enc = W_0^T dpre_0 + W_4[:, 256:]^T dpre_4 on v_mfma_f32_32x32x2_f32, then the
//                            positional encoding's Jacobian from the saved enc_x: dx (M,3)
//   composite_normals_kernel normal_map = sum_i w_i n_i, n = -g / sqrt(g.g + 1e-30), one wave per ray
//
// and the entry points: the packers, the two stages and nerf_render_normals, the render-side pass that
// chains ray features -> forward with saves -> data-gradient chain (dsigma = 1, drgb = 0) -> position
// gradient -> composite over ray chunks of at most 2^18 samples.
#include "host_api.h"
#include "train_internal.h"

namespace nerf {

// ------------------------------------------------------------------------------------ packing
// W_in[f][k]: the weight that carries input k (dpre_0's neuron k, or dpre_4's neuron k - 256) to
// encoding feature f (-1: the zero row).
NERF_HD inline float input_weight(const float* const* P, int f, int k) {
  if (f < 0) return 0.0f;
  if (k < kHidden) return P[P_PTS_W0][(size_t)k * kPosEnc + f];
  return P[2 * kSkipLayer][(size_t)(k - kHidden) * (kHidden + kPosEnc) + kHidden + f];
}

// Value of element e of the packed input-gradient weights.
NERF_HD inline float pack_input_value(const float* const* P, size_t e) {
  const int j = (int)(e & 3), lane = (int)((e >> 2) & 63);
  const int blk = (int)(e >> 8), t = blk / kInGroups, G = blk % kInGroups;
  return input_weight(P, in_row_feature(t, lane & 31), 8 * G + 4 * (lane >> 5) + j);
}

struct InputParams { const float* p[P_COUNT]; };

__global__ void __launch_bounds__(256) pack_input_kernel(InputParams P, float* __restrict__ packedIn) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < kPackedInFloats) packedIn[e] = pack_input_value(P.p, e);
}

static int launch_pack_input(const float* const* params, float* packedIn, hipStream_t s) {
  InputParams P;
  for (int i = 0; i < P_COUNT; ++i) P.p[i] = params[i];
  hipLaunchKernelGGL(pack_input_kernel, dim3((unsigned)(kPackedInFloats / 256)), dim3(256), 0, s, P, packedIn);
  return check_launch("pack_input_kernel");
}

static void pack_input_host(const float* const* params, float* packedIn) {
  for (size_t e = 0; e < kPackedInFloats; ++e) packedIn[e] = pack_input_value(params, e);
}

// --------------------------------------------------------------------------- position gradient
// One wave per block of 32 samples, four waves per workgroup.  Lane l = 32 h + s owns sample s of the
// block.  The GEMM runs as two output tiles (64 encoding rows) over the 512 inputs, dpre_0's half
// and dpre_4's half in accumulators of their own (four independent MFMA chains of 128 k-steps each,
// the chain length of the data-gradient kernels), added at the end.  Per input group a lane loads 16
// bytes of each gradient slice as they lie and one 16-byte fragment per (tile, slice) from packedIn
// (128 KiB, L2-resident, the same for every wave); the next group's loads are issued before this
// group's 16 MFMAs.  Registers: 64 accumulator + 2 x 24 operand floats, 128 VGPRs in all under the
// launch bound (four waves per SIMD, no scratch); no LDS.
//
// Epilogue (layout.h, in_out_feature): lane half h holds, for its 15 (level k = 2 kk + h, component c)
// pairs, g_sin = g_enc[3 + 6 k + c] and g_cos = g_enc[6 + 6 k + c], and reads the matching sines and
// cosines from the block's saved enc_x (features only up to 62: slot 63 is the block-exponent record).
//   p[c] = identity rows, then for kk = 0..4:  p[c] += 2^k (cos . g_sin - sin . g_cos)
// every product and sum rounded on its own, 2^k exact.  One exchange between the lane halves adds the
// even and the odd levels: dx[c] = p_h0[c] + p_h1[c].  Lane half 0 stores the three floats of its
// sample; rows past M (zero rows of the last block) store nothing.
__global__ void __launch_bounds__(256, 4)
position_grad_kernel(const float* __restrict__ packedIn, const float* __restrict__ save,
                     const float* __restrict__ grad, int64_t M, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  const int64_t blk = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
  const int64_t s0 = blk * 32;
  if (s0 >= M) return;
  const int h = lane >> 5, r = lane & 31;
  const float* __restrict__ g0 = grad + blk * 32 * (int64_t)kGradRow + r * 8 + 4 * h;   // dpre_0, group 0
  const float* __restrict__ g4 = g0 + tile_col(kSkipLayer * kHidden);                   // dpre_4, group 0
  const f32x4* __restrict__ wf = reinterpret_cast<const f32x4*>(packedIn) + lane;
  constexpr int kHalf = kInGroups / 2;   // groups per slice

  auto ldg = [&](const float* base, int G) { return *reinterpret_cast<const f32x4*>(base + (int64_t)G * 256); };
  auto ldw = [&](int t, int G) { return wf[(t * kInGroups + G) * 64]; };

  f32x16 a00{}, a01{}, a10{}, a11{};   // a<tile><slice>
  f32x4 b0 = ldg(g0, 0), b4 = ldg(g4, 0);
  f32x4 w00 = ldw(0, 0), w10 = ldw(1, 0), w01 = ldw(0, kHalf), w11 = ldw(1, kHalf);
#pragma unroll 4
  for (int G = 0; G < kHalf; ++G) {
    const int Gn = G + 1 < kHalf ? G + 1 : G;
    const f32x4 nb0 = ldg(g0, Gn), nb4 = ldg(g4, Gn);
    const f32x4 nw00 = ldw(0, Gn), nw10 = ldw(1, Gn), nw01 = ldw(0, kHalf + Gn), nw11 = ldw(1, kHalf + Gn);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a00 = mfma32t(w00[j], b0[j], a00);
      a10 = mfma32t(w10[j], b0[j], a10);
      a01 = mfma32t(w01[j], b4[j], a01);
      a11 = mfma32t(w11[j], b4[j], a11);
    }
    b0 = nb0, b4 = nb4;
    w00 = nw00, w10 = nw10, w01 = nw01, w11 = nw11;
  }
  const f32x16 t0 = a00 + a01, t1 = a10 + a11;   // value i = 16 t + g of this lane half

  // the block's saved enc_x of this lane's sample (tile-major: feature f at (f / 8) 256 + f % 8); a lane
  // half reads its own levels' 30 values, level 2 kk + h lying 6 h features behind level 2 kk
  const float* __restrict__ ex = save + blk * 32 * (int64_t)kSaveRow + tile_col(kSaveEncX) + r * 8;
  auto enc = [&](int fa, int fb) { return ex[h ? (fb / 8) * 256 + fb % 8 : (fa / 8) * 256 + fa % 8]; };
  float p[3];
  p[0] = h ? 0.0f : t1[14];
  p[1] = h ? t1[14] : 0.0f;
  p[2] = h ? 0.0f : t1[15];
  const float odd = h ? 2.0f : 1.0f;
  static_for<5>([&](auto kc) __attribute__((always_inline)) {
    constexpr int kk = decltype(kc)::value;
    const float scale = (float)(1 << (2 * kk)) * odd;   // 2^(2 kk + h)
    static_for<3>([&](auto cc) __attribute__((always_inline)) {
      constexpr int c = decltype(cc)::value;
      constexpr int i = 2 * (3 * kk + c);               // the pair's sin value; i + 1 its cos value
      const float gs = i < 16 ? t0[i % 16] : t1[i % 16], gc = i + 1 < 16 ? t0[(i + 1) % 16] : t1[(i + 1) % 16];
      constexpr int f = 3 + 12 * kk + c;                // sin feature of level 2 kk (half 1: level 2 kk + 1, + 6)
      const float sn = enc(f, f + 6), cs = enc(f + 3, f + 9);
      static_assert(f + 9 < kPosEnc, "only features are read, never enc_x's pad slot");
      p[c] = p[c] + scale * (cs * gs - sn * gc);
    });
  });
  float out[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = p[c] + __shfl_xor(p[c], 32);
  if (h == 0 && s0 + r < M) {
    float* __restrict__ o = dx + (s0 + r) * 3;
    o[0] = out[0], o[1] = out[1], o[2] = out[2];
  }
}

static int launch_position_grad(const float* packedIn, const float* save, const float* grad, int64_t M, float* dx,
                                hipStream_t s) {
  if (M == 0) return NERF_OK;
  hipLaunchKernelGGL(position_grad_kernel, dim3((unsigned)((M + 127) / 128)), dim3(256), 0, s, packedIn, save, grad, M,
                     dx);
  return check_launch("position_grad_kernel");
}

// ---------------------------------------------------------------------------- composite normals
// One wave per ray, 4 rays per workgroup, 64-sample chunks in sample order (distortion_kernel's layout).
// A lane forms w n of its sample in double from the float gradient, n = -g / sqrt(g.g + 1e-30) (g = 0:
// n = 0), and keeps its own running sum over the chunks; one butterfly at the end adds the 64 lanes in a
// fixed order and each component is rounded once.  A ray's result depends on its own samples only.
__global__ void __launch_bounds__(256)
composite_normals_kernel(const float* __restrict__ dx, const float* __restrict__ weights, int64_t B, int T,
                         float* __restrict__ normal_map) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ray >= B) return;
  const int64_t base = ray * (int64_t)T;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int i = lane; i < T; i += 64) {
    const float* __restrict__ g = dx + (base + i) * 3;
    const double gx = (double)g[0], gy = (double)g[1], gz = (double)g[2];
    const double w = (double)weights[base + i];
    const double k = -w / sqrt(gx * gx + gy * gy + gz * gz + 1e-30);
    acc[0] += k * gx;
    acc[1] += k * gy;
    acc[2] += k * gz;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += __shfl_xor(acc[c], off);
  }
  if (lane < 3) normal_map[ray * 3 + lane] = (float)(lane == 0 ? acc[0] : (lane == 1 ? acc[1] : acc[2]));
}

static int launch_composite_normals(const float* dx, const float* weights, int64_t B, int T, float* normal_map,
                                    hipStream_t s) {
  if (B == 0) return NERF_OK;
  for (int64_t r0 = 0; r0 < B; r0 += (int64_t)1 << 30) {   // (a grid dimension holds < 2^32 work-items)
    const int64_t n = imin64(B - r0, (int64_t)1 << 30);
    hipLaunchKernelGGL(composite_normals_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s,
                       dx + r0 * (int64_t)T * 3, weights + r0 * (int64_t)T, n, T, normal_map + r0 * 3);
    if (int rc = check_launch("composite_normals_kernel")) return rc;
  }
  return NERF_OK;
}

// ------------------------------------------------------------------------------ the render-side pass
constexpr int64_t kNormalsChunkSamples = (int64_t)1 << 18;   // the training step's 4,096 x 64

// Rays per chunk for T samples a ray (T <= 4096, and the launch limit is >= 4096: at least one ray)
static int64_t normals_chunk_rays(int T) {
  return imin64(kNormalsChunkSamples, nerf_render_chunk_rays(1, 0)) / T;
}

struct NormalsWs {
  float *feat, *encd, *rgb, *sigma, *dsigma, *drgb, *save, *grad, *dx;
  uint32_t* masks;
};

// One chunk's buffers (Bc rays of T samples)
static size_t normals_carve(int64_t Bc, int T, void* base, NormalsWs& w) {
  const size_t M = (size_t)Bc * T, rows = (size_t)tile_rows((int64_t)M);
  Carver c{(char*)base};
  w.feat = c.take<float>((size_t)Bc * kRayFeat * 4);
  w.encd = c.take<float>((size_t)Bc * 32 * 4);
  w.rgb = c.take<float>(M * 3 * 4);
  w.sigma = c.take<float>(M * 4);
  w.dsigma = c.take<float>(M * 4);
  w.drgb = c.take<float>(M * 3 * 4);
  w.dx = c.take<float>(M * 3 * 4);
  w.masks = c.take<uint32_t>(M * kMaskRowBytes);
  w.save = c.take<float>(rows * kSaveRow * 4);
  w.grad = c.take<float>(rows * kGradRow * 4);
  return c.at;
}

static bool normals_shape_ok(int64_t B, int T) { return B >= 0 && T >= 1 && T <= 4096; }

}  // namespace nerf

using namespace nerf;

extern "C" {

size_t nerf_packed_input_floats(void) { return kPackedInFloats; }

int nerf_pack_weights_input(const float* const* params, float* packedIn, nerf_stream_t stream) {
  REQUIRE(params && packedIn, "nerf_pack_weights_input: null pointer");
  for (int i = 0; i < P_COUNT; ++i) REQUIRE(params[i], "nerf_pack_weights_input: parameter %d is null", i);
  return launch_pack_input(params, packedIn, (hipStream_t)stream);
}

int nerf_pack_weights_input_host(const float* const* params, float* packedIn) {
  REQUIRE(params && packedIn, "nerf_pack_weights_input_host: null pointer");
  for (int i = 0; i < P_COUNT; ++i) REQUIRE(params[i], "nerf_pack_weights_input_host: parameter %d is null", i);
  pack_input_host(params, packedIn);
  return NERF_OK;
}

int nerf_mlp_position_grad(const float* packedIn, const float* save, const float* grad, int64_t M, float* dx,
                           nerf_stream_t stream) {
  REQUIRE(M >= 0, "nerf_mlp_position_grad: M=%lld", (long long)M);
  REQUIRE(M == 0 || (packedIn && save && grad && dx), "nerf_mlp_position_grad: null pointer");
  return launch_position_grad(packedIn, save, grad, M, dx, (hipStream_t)stream);
}

int nerf_composite_normals(const float* dx, const float* weights, int64_t B, int T, float* normal_map,
                           nerf_stream_t stream) {
  REQUIRE(B >= 0, "nerf_composite_normals: B=%lld", (long long)B);
  if (T < 1 || T > 4096) return set_error(NERF_ERR_UNSUPPORTED, "nerf_composite_normals: T=%d (1..4096)", T);
  REQUIRE(B == 0 || (dx && weights && normal_map), "nerf_composite_normals: null pointer");
  return launch_composite_normals(dx, weights, B, T, normal_map, (hipStream_t)stream);
}

size_t nerf_render_normals_workspace_bytes(int64_t B, int T) {
  if (!normals_shape_ok(B, T)) return 0;
  NormalsWs w;
  return normals_carve(imin64(B, normals_chunk_rays(T)), T, nullptr, w);
}

int nerf_render_normals(const float* packed, const float* packedT, const float* packedIn, const float* rays_o,
                        const float* rays_d_normalised, const float* z_vals, const float* weights, int64_t B, int T,
                        float* normal_map, void* workspace, size_t ws_bytes, nerf_stream_t stream) {
  REQUIRE(B >= 0, "nerf_render_normals: B=%lld", (long long)B);
  if (T < 1 || T > 4096) return set_error(NERF_ERR_UNSUPPORTED, "nerf_render_normals: T=%d (1..4096)", T);
  if (B == 0) return NERF_OK;
  REQUIRE(packed && packedT && packedIn && rays_o && rays_d_normalised && z_vals && weights && normal_map && workspace,
          "nerf_render_normals: null pointer");
  const int64_t chunk = normals_chunk_rays(T), Bc = imin64(B, chunk);
  NormalsWs w;
  const size_t need = normals_carve(Bc, T, workspace, w);
  REQUIRE(ws_bytes >= need, "nerf_render_normals: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  // the upstream gradient of the density: dsigma = 1, drgb = 0 (sigma does not depend on the colour branch)
  const size_t Mc = (size_t)Bc * T;
  if (hipMemsetD32Async((hipDeviceptr_t)w.dsigma, 0x3f800000, Mc, s) != hipSuccess ||
      hipMemsetAsync(w.drgb, 0, Mc * 3 * 4, s) != hipSuccess)
    return set_error(NERF_ERR_HIP, "nerf_render_normals: hipMemsetAsync failed");
  for (int64_t r0 = 0; r0 < B; r0 += chunk) {
    const int64_t n = imin64(B - r0, chunk), M = n * T;
    const float* o = rays_o + 3 * r0;
    const float* d = rays_d_normalised + 3 * r0;
    const float* z = z_vals + r0 * T;
    if (int rc = launch_ray_features(packed, d, n, nullptr, 0, w.feat, s, w.encd)) return rc;
    if (int rc = launch_mlp(packed, o, d, z, n, T, w.feat, w.rgb, w.sigma, nullptr, 0, s, w.save, w.encd, w.masks))
      return rc;
    if (int rc = launch_mlp_backward(packed, packedT, w.save, w.masks, w.sigma, w.rgb, w.dsigma, w.drgb, M, w.grad, s))
      return rc;
    if (int rc = launch_position_grad(packedIn, w.save, w.grad, M, w.dx, s)) return rc;
    if (int rc = launch_composite_normals(w.dx, weights + r0 * T, n, T, normal_map + 3 * r0, s)) return rc;
  }
  return NERF_OK;
}

}  // extern "C"
