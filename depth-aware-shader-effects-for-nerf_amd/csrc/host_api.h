// Host-side helpers of the C-ABI files (capi.hip, train_api.hip): the argument-check macro and the
// workspace carver.  No device code.
#pragma once
#include "common.h"

namespace nerf {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Hands out a workspace's regions in order, each 256-B aligned; `at` ends as the bytes needed.
// A null base only sizes (every region comes back null).
struct Carver {
  char* base;
  size_t at = 0;
  template <typename T>
  T* take(size_t bytes) {
    T* p = base ? (T*)(base + at) : nullptr;
    at += align256(bytes);
    return p;
  }
};

}  // namespace nerf

#define REQUIRE(cond, ...)                                        \
  do {                                                            \
    if (!(cond)) return set_error(NERF_ERR_BAD_ARG, __VA_ARGS__); \
  } while (0)
