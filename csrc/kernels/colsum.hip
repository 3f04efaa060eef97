// gfx950 kernel of the column sum (the bias gradient of a linear layer).
// out[c] = sum_r in[r, c] for a row-major bf16 [M, Ncol] matrix, fp32
// accumulation and output: db = sum over the batch of dY.  Each lane owns 8
// adjacent columns (one 16-B load per row), a wave 512 columns, and the rows
// of a column tile are split over `gridDim.y` workgroups (x 4 waves) so a
// batch of a few hundred rows still spreads over the whole chip.  Each
// workgroup leaves its fp32 partial row in `part[blockIdx.y]`; the last to
// arrive at the tile's ticket sums the partials in row-split order
// (deterministic: no float atomics) and re-arms the ticket for the next call.
// Hand-off of the partial rows: LITE = write-through (sc0 sc1) stores, a
// drained vmcnt and system-coherent loads in the last workgroup (no cache
// write-back or invalidate); otherwise device-scope release / acquire fences.
#include <hip/hip_runtime.h>

#include "elem.h"
#include "kernels.h"
#include "launch_util.h"
#include "xgmi_device.h"

namespace akka {

namespace {

constexpr int kCsCols = 64 * 8;  // columns per workgroup (one wave's width)
constexpr int kCsRows = 8;       // rows per lane in flight
constexpr int kCsMaxSplits = 16;

// RELU: the ReLU backward rides along -- the summed value is in[r, c] where
// act[r, c] > 0, else 0, and it is also written to gout (bf16, same layout):
// dY of the layer below the activation and its bias gradient in one pass.
__device__ __forceinline__ v4u relu_mask_bf16x8(const v4u& g, const v4u& h) {
  v4u o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t gw = g[k], hw = h[k];
    // bf16 > 0: sign bit clear and not +0 (NaN passes through as > 0 is false for NaN in fp32 too)
    const bool lo = __uint_as_float(hw << 16) > 0.f, hi = __uint_as_float(hw & 0xffff0000u) > 0.f;
    o[k] = (lo ? (gw & 0xffffu) : 0u) | (hi ? (gw & 0xffff0000u) : 0u);
  }
  return o;
}

template <bool LITE, bool RELU>
__global__ __launch_bounds__(kBlock) void colsum_bf16_kernel(float* __restrict__ out, const bf16_t* __restrict__ in,
                                                             int64_t M, int64_t ncol, float* __restrict__ part,
                                                             uint32_t* __restrict__ tickets, int32_t vec,
                                                             const bf16_t* __restrict__ act,
                                                             bf16_t* __restrict__ gout) {
  using Bf16 = Elt<bf16_t>;
  __shared__ float red[kBlock / 64][kCsCols + kCsCols / 8];
  __shared__ uint32_t last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c0 = int64_t(blockIdx.x) * kCsCols + lane * 8;
  const int64_t rows_per = (M + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = int64_t(blockIdx.y) * rows_per;
  const int64_t r1 = r0 + rows_per < M ? r0 + rows_per : M;
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.f;
  if (vec && c0 + 8 <= ncol) {
    // kCsRows rows in flight per lane before the adds
    int64_t r = r0 + wave;
    for (; r + 4 * (kCsRows - 1) < r1; r += 4 * kCsRows) {
      v4u v[kCsRows];
#pragma unroll
      for (int u = 0; u < kCsRows; ++u) v[u] = *reinterpret_cast<const v4u*>(in + (r + 4 * u) * ncol + c0);
      if constexpr (RELU) {
        v4u h[kCsRows];
#pragma unroll
        for (int u = 0; u < kCsRows; ++u) h[u] = *reinterpret_cast<const v4u*>(act + (r + 4 * u) * ncol + c0);
#pragma unroll
        for (int u = 0; u < kCsRows; ++u) {
          v[u] = relu_mask_bf16x8(v[u], h[u]);
          *reinterpret_cast<v4u*>(gout + (r + 4 * u) * ncol + c0) = v[u];
        }
      }
#pragma unroll
      for (int u = 0; u < kCsRows; ++u) Bf16::add(acc, v[u]);
    }
    for (; r < r1; r += 4) {
      v4u v = *reinterpret_cast<const v4u*>(in + r * ncol + c0);
      if constexpr (RELU) {
        v = relu_mask_bf16x8(v, *reinterpret_cast<const v4u*>(act + r * ncol + c0));
        *reinterpret_cast<v4u*>(gout + r * ncol + c0) = v;
      }
      Bf16::add(acc, v);
    }
  } else {
    for (int64_t r = r0 + wave; r < r1; r += 4)
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (c0 + q < ncol) {
          float g = Bf16::to_f(in[r * ncol + c0 + q]);
          if constexpr (RELU) {
            if (!(Bf16::to_f(act[r * ncol + c0 + q]) > 0.f)) g = 0.f;
            gout[r * ncol + c0 + q] = Bf16::from_f(g);
          }
          acc[q] += g;
        }
  }
  // the workgroup's 4 waves -> one partial row (acc[q] is column c0 + q),
  // staged with one pad word per lane (slot lane * 9 + q): a wave's stores of
  // one q are 9 words apart and the combine's reads of consecutive columns
  // are consecutive but for the pads -- no bank conflicts either way
#pragma unroll
  for (int q = 0; q < 8; ++q) red[wave][lane * 9 + q] = acc[q];
  __syncthreads();
  float* prow = part + int64_t(blockIdx.y) * ncol;
  const auto prs = xgmi::sys_rsrc(part, int64_t(gridDim.y) * ncol * 4);
  for (int i = threadIdx.x; i < kCsCols; i += kBlock) {
    const int64_t c = int64_t(blockIdx.x) * kCsCols + i;
    if (c >= ncol) continue;
    const int li = i + (i >> 3);  // column i of the tile = lane i / 8, element i % 8
    const float v = red[0][li] + red[1][li] + red[2][li] + red[3][li];
    if constexpr (LITE)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), prs, int((int64_t(blockIdx.y) * ncol + c) * 4), 0,
                                            xgmi::kSysAux);
    else
      prow[c] = v;
  }
  if constexpr (LITE) {
    xgmi::drain_wg();  // every wave's write-through stores performed
  } else {
    __threadfence();  // release: this workgroup's partial row before its ticket
    __syncthreads();
  }
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(&tickets[blockIdx.x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                   gridDim.y - 1
               ? 1u
               : 0u;
  __syncthreads();
  if (!last) return;
  if constexpr (!LITE) __threadfence();  // acquire: every partial row of this tile
  // every partial of a column loaded before the first add (one memory
  // latency for the combine, not one per split), summed in split order
  for (int i = threadIdx.x; i < kCsCols; i += kBlock) {
    const int64_t c = int64_t(blockIdx.x) * kCsCols + i;
    if (c >= ncol) continue;
    float v[kCsMaxSplits];
#pragma unroll
    for (int y = 0; y < kCsMaxSplits; ++y) {
      v[y] = 0.f;
      if (y < int(gridDim.y)) {
        if constexpr (LITE)
          v[y] = __uint_as_float(
              __builtin_amdgcn_raw_buffer_load_b32(prs, int((int64_t(y) * ncol + c) * 4), 0, xgmi::kSysAux));
        else
          v[y] = part[int64_t(y) * ncol + c];
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int y = 0; y < kCsMaxSplits; ++y) sum += v[y];
    out[c] = sum;
  }
  if (threadIdx.x == 0)  // re-armed for the next launch on this workspace
    __hip_atomic_store(&tickets[blockIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

int32_t colsum_row_splits(int64_t M, int64_t ncol) {
  const int64_t tiles = (ncol + kCsCols - 1) / kCsCols;
  // one workgroup per CU over the chip at most, >= 32 rows per workgroup
  int64_t r = (kCUs + tiles - 1) / tiles;
  const int64_t cap = M / 32;
  if (r > cap) r = cap;
  if (r > kCsMaxSplits) r = kCsMaxSplits;
  return int32_t(r < 1 ? 1 : r);
}

void launch_colsum_bf16(hipStream_t s, float* out, const void* in, int64_t M, int64_t ncol, float* part,
                        uint32_t* tickets, int32_t splits, bool lite, const void* act, void* gout) {
  if (ncol <= 0) return;
  AKKA_CHECK(M > 0 && splits >= 1 && splits <= kCsMaxSplits, "colsum: bad shape or row splits (1..16)");
  const int64_t tiles = (ncol + kCsCols - 1) / kCsCols;
  AKKA_CHECK(tiles < (int64_t(1) << 31), "colsum: too many columns");
  // the partial rows are addressed through one buffer resource (32-bit offsets)
  AKKA_CHECK(int64_t(splits) * ncol * 4 < (int64_t(1) << 31), "colsum: partial rows exceed 2 GiB");
  AKKA_CHECK((act == nullptr) == (gout == nullptr), "colsum: the ReLU mask needs both act and gout");
  const bool relu = act != nullptr;
  const int vec = ((reinterpret_cast<uintptr_t>(in) | (relu ? reinterpret_cast<uintptr_t>(act) |
                                                                   reinterpret_cast<uintptr_t>(gout)
                                                             : uintptr_t(0))) &
                   15) == 0 && ncol % 8 == 0
                      ? 1
                      : 0;
  const auto* a16 = static_cast<const bf16_t*>(act);
  auto* g16 = static_cast<bf16_t*>(gout);
  const dim3 grid{uint32_t(tiles), uint32_t(splits), 1u};
#define AKKA_CS(L, R)                                                                                              \
  hipLaunchKernelGGL((colsum_bf16_kernel<L, R>), grid, dim3(kBlock), 0, s, out, static_cast<const bf16_t*>(in), M, \
                     ncol, part, tickets, vec, a16, g16)
  if (lite) {
    if (relu) AKKA_CS(true, true);
    else AKKA_CS(true, false);
  } else {
    if (relu) AKKA_CS(false, true);
    else AKKA_CS(false, false);
  }
#undef AKKA_CS
  check_launch("colsum_bf16");
}

}  // namespace akka
