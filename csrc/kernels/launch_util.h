// What the kernel units share outside the element codec: the workgroup and
// grid constants of the streaming kernels (used by device and host code), the
// host's launch check and its compile-time-count dispatch.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../engine/common.h"

namespace akka {

constexpr int kBlock = 256;         // threads per workgroup (4 waves of 64)
constexpr int kCUs = 256;           // MI355X
constexpr int kMaxGrid = kCUs * 8;  // 256 CUs x 8 blocks

inline void check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw AkkaError(std::string("akka: ") + what + ": " + hipGetErrorString(e));
}

// Workgroups of a region walk (the kernels over per-(block, chunk) counts):
// one per region up to max_grid, and `split` workgroups sharing a region
// (gridDim.y) while there are few regions and a region has the vectors to
// keep them busy.
struct RegionGrid {
  int grid, split;
};
inline RegionGrid region_grid(int64_t regions, int64_t S, int64_t max_grid) {
  const int grid = int(regions < max_grid ? regions : max_grid);
  int split = int(max_grid / grid);
  const int64_t per_region_vecs = (S / regions) / 4 + 1;
  const int64_t useful = (per_region_vecs + kBlock - 1) / kBlock;
  if (split > useful) split = int(useful);
  if (split < 1) split = 1;
  return {grid, split};
}

// Calls f(std::integral_constant<int, K>{}) for the K among Ks that equals n;
// false (f not called) when none does.  One fold over ||: it stops at the
// first K == n; `(f(...), true)` is the built-in comma, so f may return void.
template <int... Ks, typename F>
bool dispatch_int(int n, F&& f) {
  return ((n == Ks && (f(std::integral_constant<int, Ks>{}), true)) || ...);
}

// The one-sided lanes' kernels: f(std::integral_constant<int, NS>{}) with
// NS = N for a node's rank counts (2..8, 16) and NS = 0 (runtime N) otherwise.
template <typename F>
void with_ns(int N, F&& f) {
  if (!dispatch_int<2, 3, 4, 5, 6, 7, 8, 16>(N, f)) f(std::integral_constant<int, 0>{});
}

}  // namespace akka
