// Does the immediate offset of global_load_lds_dwordx4 move the LDS destination together with the
// global address?  (CDNA ISA: LDS address = LDS base + M0[15:0] + instruction offset + 16 lane for the
// dwordx4 form; the render MLP's weight DMA, csrc/mlp16s.hip sdma_piece, relies on it.)
// One workgroup of 4 waves DMAs a known 16 KiB pattern into a 16 KiB LDS array the way the kernel
// does: wave w writes M0 once (array + 4096 w) and issues four pieces from one address pair, at
// offset:0, 1024, 2048, 3072, with voff = 16 lane + 4096 w.  The array is then copied out and
// compared with the pattern on the host.  Every address stays inside the program's own buffers
// whichever way the offset is applied: the global reads end at byte 16383 of the 16 KiB source, and
// the largest LDS address either reading gives is array + 16383.
//   hipcc --offload-arch=gfx950 -O3 -o scripts/microbench/lds_dma_offset scripts/microbench/lds_dma_offset.hip
// Prints "lds_dma_offset: OK" and exits 0 when the offset moves both, 1 otherwise (with the first
// differing word and where its value came from).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <vector>

constexpr int kWords = 4096;   // 16 KiB

__global__ void __launch_bounds__(256) dma_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWords];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < kWords; i += 256) lds[i] = 0xdeadbeefu;
  __syncthreads();
  const uint32_t dst = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + 4096u * wave;
  const uint32_t voff = 16u * lane + 4096u * wave;
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
      "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
      "global_load_lds_dwordx4 %1, %2 offset:3072\n\t"
      "s_waitcnt vmcnt(0)\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(src), "s"(dst)
      : "memory");
  __syncthreads();
  for (int i = threadIdx.x; i < kWords; i += 256) out[i] = lds[i];
}

int main() {
  std::vector<uint32_t> pattern(kWords), got(kWords);
  for (int i = 0; i < kWords; ++i) pattern[i] = 0x10000u + (uint32_t)i;   // word i names itself
  uint32_t *src, *out;
  if (hipMalloc(&src, kWords * 4) != hipSuccess || hipMalloc(&out, kWords * 4) != hipSuccess) return 2;
  (void)hipMemcpy(src, pattern.data(), kWords * 4, hipMemcpyHostToDevice);
  (void)hipMemset(out, 0, kWords * 4);
  hipLaunchKernelGGL(dma_kernel, dim3(1), dim3(256), 0, 0, src, out);
  if (hipDeviceSynchronize() != hipSuccess) {
    printf("lds_dma_offset: kernel failed: %s\n", hipGetErrorString(hipGetLastError()));
    return 2;
  }
  (void)hipMemcpy(got.data(), out, kWords * 4, hipMemcpyDeviceToHost);
  for (int i = 0; i < kWords; ++i)
    if (got[i] != pattern[i]) {
      printf("lds_dma_offset: DIFFERENT at word %d (byte %d): got 0x%x", i, 4 * i, got[i]);
      if (got[i] >= 0x10000u && got[i] < 0x10000u + kWords) printf(" = source word %u", got[i] - 0x10000u);
      printf("\n");
      return 1;
    }
  printf("lds_dma_offset: OK (the immediate offset moves the LDS destination and the global address)\n");
  return 0;
}
