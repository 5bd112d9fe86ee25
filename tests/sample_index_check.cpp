// Host build of csrc/sample_index.h (tests/test_sample_index.py compiles and runs it): the render
// MLP's sample -> ray division by a multiply-high and its exact reciprocal of a power-of-two scale,
// against `/`, `%` and the float division.  Prints one "ok <check> <cases>" line per check that
// holds and a "FAIL ..." line for the first counterexample of one that does not.
//   sample_index_check [hex bit patterns of further constants for the reciprocal check]
//   sample_index_check --layout    prints the packed buffer's offset and count of the kernel's constants
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "sample_index.h"

using namespace nerf;

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static float float_of(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rng() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// quotient and remainder of n by d through the helper, against the operators
static bool div_holds(int64_t n, int d, const RayDiv& rd, const char* what) {
  const int q = ray_div((int)n, rd.mul, rd.shift);
  const int r = (int)n - q * d;
  if (q == (int)(n / d) && r == (int)(n % d)) return true;
  printf("FAIL %s: n=%lld d=%d mul=%u shift=%d -> q=%d r=%d, / gives %lld %% gives %lld\n", what, (long long)n, d,
         rd.mul, rd.shift, q, r, (long long)(n / d), (long long)(n % d));
  return false;
}

static bool check_div_points() {
  const int64_t top = ((int64_t)1 << 31) - 1;
  std::vector<int> ds;
  for (int d = 1; d <= 4096; ++d) ds.push_back(d);
  ds.push_back(1 << 30);
  ds.push_back((int)top);
  long cases = 0;
  for (int d : ds) {
    const RayDiv rd = ray_div_of(d);
    if (rd.shift < 0 || rd.shift > 31) {
      printf("FAIL div_points: d=%d shift=%d\n", d, rd.shift);
      return false;
    }
    std::vector<int64_t> ks = {1, 2, 3, 5, 7, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 1000, 4095, 4096, 4097,
                               65535, 65536, 1 << 20, top / d - 1, top / d, top / d + 1, top / d / 2, top / d / 3};
    for (int i = 0; i < 16; ++i) ks.push_back((int64_t)(rng() % (uint64_t)(top / d + 1)));
    std::vector<int64_t> ns = {0, (int64_t)d - 1, d, top, top - 1};
    for (int64_t k : ks)
      for (int64_t n : {k * d - 1, k * d, k * d + 1}) ns.push_back(n);
    for (int64_t n : ns) {
      if (n < 0 || n > top) continue;
      if (!div_holds(n, d, rd, "div_points")) return false;
      ++cases;
    }
  }
  printf("ok div_points %ld\n", cases);
  return true;
}

// the samples a wave meets: block b, b + grid, ... of 128 samples, 10,000 steps of three grid sizes,
// the wave's first and last lanes of both sample tiles
static bool check_div_steps() {
  long cases = 0;
  for (int grid : {1, 256, 304})
    for (int d : {1, 7, 32, 33, 64, 192, 1000}) {
      const RayDiv rd = ray_div_of(d);
      int64_t blk = grid - 1;
      for (int step = 0; step < 10000; ++step, blk += grid)
        for (int wave : {0, 3})
          for (int off : {0, 15, 16, 31}) {
            const int64_t n = (blk * 4 + wave) * 32 + off;
            if (n >= ((int64_t)1 << 31)) {
              printf("FAIL div_steps: sample %lld out of range\n", (long long)n);
              return false;
            }
            if (!div_holds(n, d, rd, "div_steps")) return false;
            ++cases;
          }
    }
  printf("ok div_steps %ld\n", cases);
  return true;
}

// c / s == c * pow2_recip(s), bit for bit, for every scale stream16.h's pow2_scale returns (2^(14 - e),
// e clamped to -100 .. 100) and: the constants given on the command line, 10^6 random constants whose
// quotient is normal (magnitudes 2^-12 .. 2^41, the division's domain in the kernel: its constants are
// 2^(e_w - 14) of a weight maximum), zero, and 10^6 random bit patterns of any kind (both sides are the
// correctly rounded c 2^-k, so they agree on subnormal and overflowing results too; NaN matches NaN)
static bool recip_holds(float c, float s) {
  const float q = c / s, p = c * pow2_recip(s);
  if (bits_of(q) == bits_of(p) || (q != q && p != p)) return true;
  printf("FAIL recip: c=%08x s=%08x: c / s = %08x, c * recip = %08x\n", bits_of(c), bits_of(s), bits_of(q), bits_of(p));
  return false;
}
static bool check_recip(int argc, char** argv) {
  std::vector<float> cs = {0.0f, -0.0f, 1.0f};
  for (int i = 1; i < argc; ++i) cs.push_back(float_of((uint32_t)strtoul(argv[i], nullptr, 16)));
  const size_t given = cs.size();
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t r = rng();
    const uint32_t ex = 127 - 12 + (uint32_t)((r >> 32) % 53);   // biased exponent of 2^-12 .. 2^40
    cs.push_back(float_of((uint32_t)(r & 0x807FFFFFu) | (ex << 23)));
  }
  for (int i = 0; i < 1000000; ++i) cs.push_back(float_of((uint32_t)rng()));
  long cases = 0;
  for (int e = -100; e <= 100; ++e) {
    const float s = ldexpf(1.0f, 14 - e);
    if (pow2_recip(s) != ldexpf(1.0f, e - 14)) {
      printf("FAIL recip: e=%d recip=%08x\n", e, bits_of(pow2_recip(s)));
      return false;
    }
    // every scale on the given and the normal-range constants; the arbitrary bit patterns on a
    // rotating tenth of the scales
    for (size_t i = 0; i < cs.size(); ++i) {
      if (i >= given + 1000000 && (int)(i % 10) != (e + 100) % 10) continue;
      if (!recip_holds(cs[i], s)) return false;
      ++cases;
    }
  }
  printf("ok recip %ld given %zu\n", cases, given - 3);
  return true;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--layout")) {   // where the packed buffer keeps the divided constants
    printf("invw %zu %d\n", (size_t)kOffScale16 + kS16InvW, 9);
    return 0;
  }
  bool ok = check_div_points();
  ok = check_div_steps() && ok;
  ok = check_recip(argc, argv) && ok;
  return ok ? 0 : 1;
}
