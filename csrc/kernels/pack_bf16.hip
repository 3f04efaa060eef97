// gfx950 kernel of the compressed gradient wire: fp32 -> bf16 pack with error
// feedback.
// q[i] = bf16_rne(e), e = g[i] + r[i]; r[i] = e - float(q[i]) in place (RES),
// e = g[i] without a residual.  No multiply, so nothing contracts: g + r and
// e - q are one IEEE fp32 operation each and float(q) + r == e exactly for
// finite values.  Where e or q is not finite (a finite e may round to +-inf)
// q is stored as is and r becomes 0, so one overflow does not stay in r.
// head: elements below the first one that is 16-B aligned in all three
// streams; block 0 does head and tail.  head < 0: the streams share no such
// element, every element goes through the scalar path.  The body is units of
// 8 elements: two 16-B loads of g (and of r) per 16-B store of q, 8 loads in
// flight per thread before the first store (as count_mean's AXPY group).
// NT: nontemporal loads and stores for streams past the Infinity Cache.
#include <hip/hip_runtime.h>

#include "elem.h"
#include "kernels.h"
#include "launch_util.h"

namespace akka {

namespace {

template <bool RES>
__device__ __forceinline__ bf16_t pack_one(float g, float& r) {
  const float e = RES ? g + r : g;
  const bf16_t q = Elt<bf16_t>::from_f(e);
  if constexpr (RES) {
    const float f = Elt<bf16_t>::to_f(q);
    // finite: exponent not all ones (f is inf or NaN whenever e is; f alone may be inf)
    const bool fin = (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u;
    r = fin ? e - f : 0.f;
  }
  return q;
}

template <bool RES, bool NT>
__global__ __launch_bounds__(kBlock) void pack_bf16_kernel(bf16_t* __restrict__ q, const float* __restrict__ g,
                                                           float* r, int64_t n, int64_t head) {
  auto one = [&](int64_t i) {
    float rr = RES ? r[i] : 0.f;
    q[i] = pack_one<RES>(g[i], rr);
    if constexpr (RES) r[i] = rr;
  };
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  if (head < 0) {
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) one(i);
    return;
  }
  const int64_t nunit = (n - head) / 8;
  if (blockIdx.x == 0) {
    for (int64_t i = threadIdx.x; i < head; i += kBlock) one(i);
    for (int64_t i = head + nunit * 8 + threadIdx.x; i < n; i += kBlock) one(i);
  }
  const v4u* g4 = reinterpret_cast<const v4u*>(g + head);
  v4u* r4 = reinterpret_cast<v4u*>(r + head);
  v4u* q4 = reinterpret_cast<v4u*>(q + head);
  auto ld = [](const v4u* p) { return NT ? __builtin_nontemporal_load(p) : *p; };
  auto st = [](const v4u& x, v4u* p) {
    if constexpr (NT) __builtin_nontemporal_store(x, p);
    else *p = x;
  };
  constexpr int U = RES ? 2 : 4;
  for (int64_t base = int64_t(blockIdx.x) * kBlock + threadIdx.x; base < nunit; base += stride * U) {
    v4u gv[U][2], rv[U][2];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * stride;
      if (i < nunit) {
        gv[u][0] = ld(g4 + 2 * i);
        gv[u][1] = ld(g4 + 2 * i + 1);
        if constexpr (RES) {
          rv[u][0] = ld(r4 + 2 * i);
          rv[u][1] = ld(r4 + 2 * i + 1);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * stride;
      if (i < nunit) {
        bf16_t h[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float rr = RES ? __uint_as_float(rv[u][k >> 2][k & 3]) : 0.f;
          h[k] = pack_one<RES>(__uint_as_float(gv[u][k >> 2][k & 3]), rr);
          if constexpr (RES) rv[u][k >> 2][k & 3] = __float_as_uint(rr);
        }
        if constexpr (RES) {
          st(rv[u][0], r4 + 2 * i);
          st(rv[u][1], r4 + 2 * i + 1);
        }
        st(v4u{uint32_t(h[0]) | uint32_t(h[1]) << 16, uint32_t(h[2]) | uint32_t(h[3]) << 16,
               uint32_t(h[4]) | uint32_t(h[5]) << 16, uint32_t(h[6]) | uint32_t(h[7]) << 16},
           q4 + i);
      }
    }
  }
}

}  // namespace

void launch_pack_bf16(hipStream_t s, void* q, const float* g, float* r, int64_t n) {
  if (n <= 0) return;
  AKKA_CHECK((reinterpret_cast<uintptr_t>(q) & 1) == 0 && (reinterpret_cast<uintptr_t>(g) & 3) == 0 &&
                 (reinterpret_cast<uintptr_t>(r) & 3) == 0,
             "pack_bf16: buffers must be aligned to their element size");
  // first element at which q, g and r are all 16-B aligned, if they share one
  int64_t head = -1;
  for (int64_t h = 0; h < 8 && head < 0; ++h) {
    const bool ok = ((reinterpret_cast<uintptr_t>(q) + 2 * h) & 15) == 0 &&
                    ((reinterpret_cast<uintptr_t>(g) + 4 * h) & 15) == 0 &&
                    (r == nullptr || ((reinterpret_cast<uintptr_t>(r) + 4 * h) & 15) == 0);
    if (ok) head = h;
  }
  if (head > n) head = n;
  // Cache policy and grid as the one-source reduce: everything fits the
  // Infinity Cache -> plain accesses (the round reads q next), a grid over the
  // whole stream; larger -> nontemporal loads and stores, 2 blocks/CU.
  const int64_t bytes = n * (r ? 14 : 6);
  const bool nt = bytes > (int64_t(256) << 20);
  const int64_t per_block = int64_t(kBlock) * (head < 0 ? 1 : 8 * (r ? 2 : 4));
  const int64_t cap = int64_t(kCUs) * (nt ? 2 : 16);
  const int64_t want = (n + per_block - 1) / per_block;
  const int grid = int(want < cap ? want : cap);
#define AKKA_PK(RES, NT)                                                                               \
  hipLaunchKernelGGL((pack_bf16_kernel<RES, NT>), dim3(grid), dim3(kBlock), 0, s, static_cast<bf16_t*>(q), g, r, n, \
                     head)
  if (r) {
    if (nt) AKKA_PK(true, true);
    else AKKA_PK(true, false);
  } else {
    if (nt) AKKA_PK(false, true);
    else AKKA_PK(false, false);
  }
#undef AKKA_PK
  check_launch("pack_bf16");
}

}  // namespace akka
