// Prints csrc/composite_plan.h's decisions over a table of cases, one line per case, for
// tests/test_composite_plan.py (a plain host program: the header has no HIP types).
//   fwd <B> <N> <Nf> <merged> <rgb> <sigma> <z> <weights> <bg> : <plan>     (pointers as byte offsets from a
//   bwd <B> <N> <Nf> <merged> <acc> : <plan>                                 16-byte boundary, -1 = null)
//   <plan> = <skip|launch|refuse> <vec> <merged> <stage> <alt> <grid> <block> <lds> <name>
#include <cstdio>
#include <initializer_list>

#include "composite_plan.h"

using namespace nerf;

static void print_plan(const CompositePlan& p) {
  static const char* const actions[] = {"skip", "launch", "refuse"};
  std::printf(" : %s %d %d %d %d %u %u %zu %s\n", actions[p.action], (int)p.vec, (int)p.merged, (int)p.stage, (int)p.alt,
              p.grid, p.block, p.lds, p.name);
}

static const void* at(int off) { return off < 0 ? nullptr : (const void*)(uintptr_t)(0x10000 + off); }

static void fwd(long long B, int N, int Nf, int merged, int rgb, int sigma, int z, int weights, int bg) {
  std::printf("fwd %lld %d %d %d %d %d %d %d %d", B, N, Nf, merged, rgb, sigma, z, weights, bg);
  print_plan(composite_forward_plan(B, N, Nf, merged, at(rgb), at(sigma), at(z), at(weights), bg));
}

static void bwd(long long B, int N, int Nf, int merged, int acc) {
  std::printf("bwd %lld %d %d %d %d", B, N, Nf, merged, acc);
  print_plan(composite_backward_plan(B, N, Nf, merged, acc));
}

int main() {
  const long long Bs[] = {0, 1, 3, 4, 5, 16, 17};
  // every pointer aligned; rgb, sigma, z, weights in turn off by 4 bytes; weights null
  const int dense_ptrs[][4] = {{0, 0, 0, 0}, {4, 0, 0, 0}, {0, 4, 0, 0}, {0, 0, 4, 0}, {0, 0, 0, 4}, {0, 0, 0, -1}};
  const int merged_shapes[][2] = {{7, 6}, {8, 8}, {64, 192}, {64, 193}, {64, 196}, {64, 197}};   // T = 13 .. 261
  const int bwd_shapes[][2] = {{1, 1}, {256, 512}, {256, 513}, {256, 1024}, {257, 1024}, {8, 0}, {0, 8}};
  for (long long B : Bs)
    for (int bg = 0; bg < 2; ++bg) {
      for (int N : {1, 4, 7, 8, 68, 4096})
        for (const auto& o : dense_ptrs) fwd(B, N, 0, 0, o[0], o[1], o[2], o[3], bg);
      // the merged form never looks at rgb / sigma (here misaligned): z_all and weights decide
      for (const auto& n : merged_shapes)
        for (int z : {0, 4})
          for (int weights : {0, 4, -1}) fwd(B, n[0], n[1], 1, 4, 4, z, weights, bg);
    }
  for (long long B : Bs)
    for (int acc = 0; acc < 2; ++acc) {
      for (int N : {1, 7, 68, 4096}) bwd(B, N, 0, 0, acc);
      for (const auto& n : bwd_shapes) bwd(B, n[0], n[1], 1, acc);
    }
  return 0;
}
