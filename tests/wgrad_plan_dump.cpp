// Prints csrc/wgrad_plan.h's decisions over a grid of shapes, one line per case, for
// tests/test_wgrad_plan.py (a plain host program: the header has no HIP types).
//   plan <arith> <N> <K> <x_div> <M> <lda> <ldx> <aligned> <tiled> <x_tiled> : <route> <clen> <chunks>
//        <x_blk> <xd1> <scaled> <writes_sums> <partial_floats> <wgrad_workspace_floats(M, N, K)>
//   head3 <M> <chunks * stride> <wgrad_stream_floats(M)>     (the rgb head's streaming launch)
//   pair <M> <clen> <chunks * stride> <wgrad_stream_floats(M)>   (the layer-0 / skip-PE pair)
#include <cstdio>

#include "wgrad_plan.h"

using namespace nerf;

static const char* route_name(WgradRoute r) {
  switch (r) {
    case WgradRoute::Fallback: return "fallback";
    case WgradRoute::Lds128x128: return "lds128x128";
    case WgradRoute::Lds256x64: return "lds256x64";
    case WgradRoute::Bf128x128: return "bf128x128";
    case WgradRoute::Bf256x64: return "bf256x64";
    case WgradRoute::BfK64: return "bfk64";
    case WgradRoute::H16Whole: return "h16whole";
    case WgradRoute::H16Half: return "h16half";
  }
  return "?";
}

static void plan_line(int arith, int N, int K, long long x_div, long long M, long long lda, long long ldx, int aligned,
                      int tiled, int x_tiled) {
  const WgradPlan p = wgrad_plan(arith, N, K, x_div, M, lda, ldx, aligned, tiled, x_tiled);
  std::printf("plan %d %d %d %lld %lld %lld %lld %d %d %d : %s %d %d %d %d %d %d %zu %zu\n", arith, N, K, x_div, M, lda,
              ldx, aligned, tiled, x_tiled, route_name(p.route), p.clen, p.chunks, (int)p.x_blk, (int)p.xd1,
              (int)p.scaled, (int)p.writes_sums, p.partial_floats, wgrad_workspace_floats(M, N, K));
}

int main() {
  const int Ns[] = {1, 3, 5, 33, 64, 65, 125, 128, 160, 256, 512};
  const int Ks[] = {0, 1, 9, 27, 32, 62, 63, 64, 65, 70, 128, 256, 288, 319};
  const long long divs[] = {0, 1, 2, 8, 64};
  const long long Ms[] = {1, 17, 33, 700, 4099, 32768, 262144, 262147};
  const long long big = 1ll << 18;
  const long long lds[][2] = {{2400, 2400}, {big, 2400}, {2400, big}, {big, big}};
  for (int arith = 0; arith < 2; ++arith)
    for (int N : Ns)
      for (int K : Ks)
        for (long long x_div : divs)
          for (long long M : Ms)
            for (const auto& ld : lds)
              for (int flags = 0; flags < 8; ++flags)
                plan_line(arith, N, K, x_div, M, ld[0], ld[1], flags & 1, (flags >> 1) & 1, (flags >> 2) & 1);
  // the production step's per-ray GEMMs (M / 8 and M / 32 rows)
  plan_line(1, 128, 27, 8, 32768, 128, 32, 1, 0, 1);
  plan_line(1, 128, 32, 2, 8192, 128, 32, 1, 0, 0);
  for (long long M : Ms) {
    std::printf("head3 %lld %zu %zu\n", M, (size_t)wgrad_head3_chunks(M) * (size_t)wgrad_stride(3, kDirHidden),
                wgrad_stream_floats(M));
    std::printf("pair %lld %d %zu %zu\n", M, wgrad_pair_clen(M),
                (size_t)wgrad_pair_chunks(M) * (size_t)wgrad_stride(2 * kHidden, kPosEnc), wgrad_stream_floats(M));
  }
  return 0;
}
