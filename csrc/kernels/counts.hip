// gfx950 kernels over the per-(block, chunk) contributor counts of a round:
// the count expansion of ReducedDataBuffer.getWithCounts (RB:41-47), the
// count-weighted mean with the fused SGD update, and the fill / poison of a
// counts table behind a one-sided round.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include <cstdlib>

#include "elem.h"
#include "kernels.h"
#include "launch_util.h"

namespace akka {

namespace {

// One workgroup per (block, chunk) region at a time: the count is a
// wave-uniform scalar and the region is filled with 16-B stores (scalar head /
// tail where the region is not 16-B aligned); no per-element division.
__global__ __launch_bounds__(kBlock) void count_expand_kernel(int32_t* __restrict__ out,
                                                              const int32_t* __restrict__ counts, int64_t S,
                                                              int64_t step, int32_t N, int64_t C, int32_t kmax) {
  const int64_t nregions = int64_t(N) * kmax;
  for (int64_t reg = blockIdx.x; reg < nregions; reg += gridDim.x) {
    const int32_t j = int32_t(reg / kmax);
    const int64_t k = reg - int64_t(j) * kmax;
    const int64_t bs = j * step < S ? j * step : S;
    const int64_t be = j >= N - 1 ? S : ((j + 1) * step < S ? (j + 1) * step : S);
    const int64_t s = bs + k * C;
    if (s >= be) continue;
    const int64_t e = s + C < be ? s + C : be;
    const int32_t v = counts[reg];
    int64_t a = (s + 3) & ~int64_t(3);  // first 16-B aligned element
    if (a > e) a = e;
    const int64_t nv = (e - a) >> 2;
    if (blockIdx.y == 0) {
      for (int64_t i = s + threadIdx.x; i < a; i += kBlock) out[i] = v;
      for (int64_t i = a + nv * 4 + threadIdx.x; i < e; i += kBlock) out[i] = v;
    }
    int4* o4 = reinterpret_cast<int4*>(out + a);
    const int4 vv = make_int4(v, v, v, v);
    // gridDim.y workgroups share one region when there are few regions
    for (int64_t i = int64_t(blockIdx.y) * kBlock + threadIdx.x; i < nv; i += int64_t(kBlock) * gridDim.y) o4[i] = vv;
  }
}

// dst[i] = src[i] / count(block(i), chunk(i)), 0 where the count is 0: the
// count-weighted mean of an allreduce output (AllReduceOutput.mean) in one
// pass, reading the tiny per-chunk count table instead of a per-element one.
// Same region walk as count_expand (one wave-uniform count per region),
// spelled out in both on purpose: moved into a force-inlined helper (out
// parameter or callback alike) the same arithmetic reaches the scheduler in
// another order and these kernels, the SGD update's hot path, come out with a
// different instruction stream.
// AXPY: dst[i] += alpha * mean[i] instead (the SGD update fused into the
// averaging: one read of the sum, one read + write of the parameters).
// SHADOW (fp32 AXPY only): the updated parameters are also stored as bf16 into
// `shadow` (same element index), so a bf16 forward reads a weight copy the
// update already wrote instead of casting 4 B/element again every step.
// dst may alias src (mean(out=data): a gradient bucket averaged in place);
// each element is read before the same thread writes it, so no __restrict__.
constexpr int kCmUnroll = 4;

// TS is the source's element type, TD the destination's.  TD == TS for the
// plain passes; TD = float, TS = bf16 reads a bf16 sum (compressed wire) into
// fp32 parameters.  A vector unit is one 16-B source vector: E = 8 bf16 against
// two fp32 destination vectors in the mixed pass, so every stream keeps 16-B
// accesses.  The per-element arithmetic is shared, so a source that is exact
// in bf16 gives the same bits through either source type.
template <typename TD, typename TS, bool AXPY, bool SHADOW>
__global__ __launch_bounds__(kBlock) void count_mean_kernel(TD* dst, const TS* src,
                                                            const int32_t* __restrict__ counts, int64_t S,
                                                            int64_t step, int32_t N, int64_t C, int32_t kmax,
                                                            float alpha, bf16_t* __restrict__ shadow) {
  static_assert(!SHADOW || (AXPY && std::is_same_v<TD, float>), "shadow: fp32 SGD update only");
  constexpr int E = Elt<TS>::kPerVec;   // elements per unit
  constexpr int ED = Elt<TD>::kPerVec;  // elements per destination vector
  constexpr int ND = E / ED;            // destination vectors per unit
  static_assert(ND >= 1 && ND * ED == E, "the source type is never wider than the destination's");
  const int64_t nregions = int64_t(N) * kmax;
  for (int64_t reg = blockIdx.x; reg < nregions; reg += gridDim.x) {
    const int32_t j = int32_t(reg / kmax);
    const int64_t k = reg - int64_t(j) * kmax;
    const int64_t bs = j * step < S ? j * step : S;
    const int64_t be = j >= N - 1 ? S : ((j + 1) * step < S ? (j + 1) * step : S);
    const int64_t s = bs + k * C;
    if (s >= be) continue;
    const int64_t e = s + C < be ? s + C : be;
    const int32_t v = counts[reg];
    const float fv = float(v);
    int64_t a = (s + E - 1) & ~int64_t(E - 1);  // first element 16-B aligned in every stream
    if (a > e) a = e;
    const int64_t nv = (e - a) / E;
    auto one = [&](int64_t i) {
      const float m = v > 0 ? Elt<TS>::to_f(src[i]) / fv : 0.f;
      const float r = AXPY ? Elt<TD>::to_f(dst[i]) + alpha * m : m;
      dst[i] = Elt<TD>::from_f(r);
      if constexpr (SHADOW) shadow[i] = Elt<bf16_t>::from_f(r);
    };
    if (blockIdx.y == 0) {
      for (int64_t i = s + threadIdx.x; i < a; i += kBlock) one(i);
      for (int64_t i = a + nv * E + threadIdx.x; i < e; i += kBlock) one(i);
    }
    const v4u* s4 = reinterpret_cast<const v4u*>(src + a);
    v4u* d4 = reinterpret_cast<v4u*>(dst + a);
    struct DVec {
      v4u v[ND];
    };
    auto load_d = [&](int64_t at) {
      DVec d;
#pragma unroll
      for (int k2 = 0; k2 < ND; ++k2) d.v[k2] = d4[at * ND + k2];
      return d;
    };
    auto mean_vec = [&](const v4u& sv, const DVec& dv, int64_t at) {
      float acc[E];
#pragma unroll
      for (int q = 0; q < E; ++q) acc[q] = 0.f;
      Elt<TS>::add(acc, sv);
#pragma unroll
      for (int q = 0; q < E; ++q) acc[q] = v > 0 ? acc[q] / fv : 0.f;
      if constexpr (AXPY) {
        float p[E];
#pragma unroll
        for (int q = 0; q < E; ++q) p[q] = 0.f;
#pragma unroll
        for (int k2 = 0; k2 < ND; ++k2) Elt<TD>::add(reinterpret_cast<float(&)[ED]>(p[k2 * ED]), dv.v[k2]);
#pragma unroll
        for (int q = 0; q < E; ++q) acc[q] = p[q] + alpha * acc[q];
      }
      if constexpr (SHADOW) {
        // 4 bf16 per fp32 vector: 8 B per unit of the fp32 pass, 16 B of the mixed one
        if constexpr (E == 4) {
          reinterpret_cast<uint2*>(shadow + a)[at] =
              make_uint2(Elt<bf16_t>::pack2(acc[0], acc[1]), Elt<bf16_t>::pack2(acc[2], acc[3]));
        } else {
          reinterpret_cast<v4u*>(shadow + a)[at] = Elt<bf16_t>::pack(acc);
        }
      }
#pragma unroll
      for (int k2 = 0; k2 < ND; ++k2) d4[at * ND + k2] = Elt<TD>::pack(reinterpret_cast<const float(&)[ED]>(acc[k2 * ED]));
    };
    // kCmUnroll units per thread: every load of the group in flight before
    // the first store (one vector at a time left the pass latency-bound)
    constexpr int U = kCmUnroll;
    const int64_t stride = int64_t(kBlock) * gridDim.y;
    int64_t i = int64_t(blockIdx.y) * kBlock + threadIdx.x;
    for (; i + (U - 1) * stride < nv; i += U * stride) {
      v4u sv[U];
      DVec dv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) sv[u] = s4[i + u * stride];
      if constexpr (AXPY) {
#pragma unroll
        for (int u = 0; u < U; ++u) dv[u] = load_d(i + u * stride);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) mean_vec(sv[u], dv[u], i + u * stride);
    }
    for (; i < nv; i += stride) {
      DVec dv;
      if constexpr (AXPY) dv = load_d(i);
      mean_vec(s4[i], dv, i);
    }
  }
}

// A failed one-sided round (ipc lane wait timed out / aborted): every count
// of the round becomes 0, so the output is never handed back as exact.
__global__ void poison_counts_kernel(const uint32_t* flag, int32_t* counts, int64_t n) {
  if (__hip_atomic_load(const_cast<uint32_t*>(flag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) return;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    counts[i] = 0;
}

// An exact round's counts table in one launch: value everywhere, or 0 when
// the lane's error word is set by the time the stream gets here.
__global__ void fill_counts_kernel(const uint32_t* flag, int32_t* counts, int64_t n, int32_t value) {
  const int32_t v =
      __hip_atomic_load(const_cast<uint32_t*>(flag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0 ? value : 0;
  for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    counts[i] = v;
}

}  // namespace

void launch_fill_counts(hipStream_t s, const uint32_t* flag, int32_t* counts, int32_t value, int64_t n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(fill_counts_kernel, dim3(unsigned(std::min<int64_t>(64, (n + 255) / 256))), dim3(256), 0, s,
                     flag, counts, n, value);
}

void launch_poison_counts(hipStream_t s, const uint32_t* flag, int32_t* counts, int64_t n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(poison_counts_kernel, dim3(unsigned(std::min<int64_t>(64, (n + 255) / 256))), dim3(256), 0, s,
                     flag, counts, n);
}

void launch_count_expand(hipStream_t s, int32_t* out, const CountsTable& t) {
  if (t.S <= 0) return;
  t.check("count_expand");
  // out must be 16-B aligned for the vector stores (torch allocations are)
  AKKA_CHECK((reinterpret_cast<uintptr_t>(out) & 15) == 0, "count_expand: output not 16-B aligned");
  const auto [grid, split] = region_grid(t.regions(), t.S, kMaxGrid);
  hipLaunchKernelGGL(count_expand_kernel, dim3(grid, split), dim3(kBlock), 0, s, out, t.counts, t.S, t.step, t.N, t.C,
                     t.kmax);
  check_launch("count_expand");
}

void launch_count_mean(hipStream_t s, void* dst, const void* src, const CountsTable& t, DType dt, DType src_dt,
                       bool axpy, float alpha, void* shadow) {
  if (t.S <= 0) return;
  t.check("count_mean");
  AKKA_CHECK(src_dt == dt || (dt == DType::F32 && src_dt == DType::BF16),
             "count_mean: the source is the destination's dtype, or bf16 into fp32");
  AKKA_CHECK((reinterpret_cast<uintptr_t>(dst) & 15) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0,
             "count_mean: buffers must be 16-B aligned");
  AKKA_CHECK(shadow == nullptr || (axpy && dt == DType::F32 && (reinterpret_cast<uintptr_t>(shadow) & 15) == 0),
             "count_mean: a bf16 shadow needs the fp32 SGD update and a 16-B aligned buffer");
  // workgroups over the whole pass (AKKA_CM_MAXGRID: measurement knob)
  static const int64_t max_grid = [] {
    const char* v = std::getenv("AKKA_CM_MAXGRID");
    return v && std::atoll(v) > 0 ? int64_t(std::atoll(v)) : int64_t(kMaxGrid);
  }();
  const auto [grid, split] = region_grid(t.regions(), t.S, max_grid);
#define AKKA_CM(TD, TS, AX, SH)                                                                               \
  hipLaunchKernelGGL((count_mean_kernel<TD, TS, AX, SH>), dim3(grid, split), dim3(kBlock), 0, s,               \
                     static_cast<TD*>(dst), static_cast<const TS*>(src), t.counts, t.S, t.step, t.N, t.C, t.kmax, \
                     alpha, static_cast<bf16_t*>(shadow))
  if (dt == DType::F32 && src_dt == DType::BF16) {
    if (shadow) AKKA_CM(float, bf16_t, true, true);
    else if (axpy) AKKA_CM(float, bf16_t, true, false);
    else AKKA_CM(float, bf16_t, false, false);
  } else if (dt == DType::F32) {
    if (shadow) AKKA_CM(float, float, true, true);
    else if (axpy) AKKA_CM(float, float, true, false);
    else AKKA_CM(float, float, false, false);
  } else {
    if (axpy) AKKA_CM(bf16_t, bf16_t, true, false);
    else AKKA_CM(bf16_t, bf16_t, false, false);
  }
#undef AKKA_CM
  check_launch("count_mean");
}

}  // namespace akka
