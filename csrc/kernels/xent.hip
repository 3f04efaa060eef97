// gfx950 kernels of the fused cross entropy (the MLP's loss).
// Forward: one workgroup per row of bf16 logits [B, C]: lse = log sum exp,
// loss_r = lse - x[y_r] (0 for a label outside [0, C): torch's ignore_index),
// lse kept for the backward; the mean over the valid rows is combined by the
// last-arriving workgroup (write-through per-row words, drained vmcnt, relaxed
// ticket, system-coherent loads: the colsum hand-off) in row order.
// Backward: grad[r, c] = (exp(x - lse_r) - [c == y_r]) * go / nvalid, bf16.
// Replaces autocast's fp32 upcast + log_softmax + nll_loss (+ their
// backwards and the bf16 downcast of the gradient): two launches instead of
// six, logits read once per pass.
#include <hip/hip_runtime.h>

#include "elem.h"
#include "kernels.h"
#include "launch_util.h"
#include "xgmi_device.h"

namespace akka {

namespace {

using Bf16 = Elt<bf16_t>;

__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(v, o, 64);
    v = is_max ? fmaxf(v, w) : v + w;
  }
  __syncthreads();  // red may still be read by a previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < int(blockDim.x >> 6); ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

constexpr int64_t kIgnoreIndex = -100;  // torch's default ignore_index

__global__ __launch_bounds__(kBlock) void xent_fwd_kernel(const bf16_t* __restrict__ x, const int64_t* __restrict__ y,
                                                          int64_t B, int64_t C, float* __restrict__ lse,
                                                          float* __restrict__ rowloss, float* __restrict__ out,
                                                          uint32_t* __restrict__ ticket) {
  __shared__ float red[kBlock / 64 + 1];
  const int64_t r = blockIdx.x;
  const bf16_t* row = x + r * C;
  float m = -INFINITY;
  for (int64_t c = threadIdx.x; c < C; c += kBlock) m = fmaxf(m, Bf16::to_f(row[c]));
  m = block_reduce(m, red, true);
  float sum = 0.f;
  for (int64_t c = threadIdx.x; c < C; c += kBlock) sum += __expf(Bf16::to_f(row[c]) - m);
  sum = block_reduce(sum, red, false);
  const auto rs = xgmi::sys_rsrc(rowloss, B * 8);
  if (threadIdx.x == 0) {
    const float l = m + __logf(sum);
    const int64_t t = y[r];
    const bool valid = t >= 0 && t < C;
    // torch ignores ignore_index (-100) only; any other label outside [0, C)
    // is an error there: here the row is flagged (-1) and the loss is NaN
    const float flag = valid ? 1.f : (t == kIgnoreIndex ? 0.f : -1.f);
    lse[r] = l;
    // [loss, flag] per row, written through for the last arriver
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(valid ? l - Bf16::to_f(row[t]) : 0.f), rs, int(r * 8), 0,
                                          xgmi::kSysAux);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(flag), rs, int(r * 8 + 4), 0, xgmi::kSysAux);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    red[kBlock / 64] =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == uint32_t(B - 1) ? 1.f : 0.f;
  }
  __syncthreads();
  if (red[kBlock / 64] == 0.f) return;
  // last workgroup: mean over the valid rows, in row order per thread, then
  // a fixed-order tree across threads (deterministic)
  float ls = 0.f, nv = 0.f, nb = 0.f;
  for (int64_t i = threadIdx.x; i < B; i += kBlock) {
    ls += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, int(i * 8), 0, xgmi::kSysAux));
    const float f = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, int(i * 8 + 4), 0, xgmi::kSysAux));
    nv += f > 0.f ? f : 0.f;
    nb += f < 0.f ? 1.f : 0.f;
  }
  ls = block_reduce(ls, red, false);
  nv = block_reduce(nv, red, false);
  nb = block_reduce(nb, red, false);
  if (threadIdx.x == 0) {
    // torch: NaN when every row is ignored; NaN (and the bad-label count) when a label is out of range
    out[0] = (nv > 0.f && nb == 0.f) ? ls / nv : __uint_as_float(0x7fc00000u);
    out[1] = nv;
    out[2] = nb;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(kBlock) void xent_bwd_kernel(const bf16_t* __restrict__ x, const int64_t* __restrict__ y,
                                                          int64_t C, const float* __restrict__ lse,
                                                          const float* __restrict__ stat,  // [loss, nvalid]
                                                          const float* __restrict__ go, bf16_t* __restrict__ gx) {
  const int64_t r = blockIdx.x;
  const int64_t t = y[r];
  const float nv = stat[1];
  const float scale = (t >= 0 && t < C && nv > 0.f && stat[2] == 0.f) ? go[0] / nv : 0.f;
  const float l = lse[r];
  const bf16_t* row = x + r * C;
  bf16_t* g = gx + r * C;
  for (int64_t c = threadIdx.x; c < C; c += kBlock) {
    const float p = __expf(Bf16::to_f(row[c]) - l) - (c == t ? 1.f : 0.f);
    g[c] = Bf16::from_f(p * scale);
  }
}

}  // namespace

void launch_xent_fwd(hipStream_t s, const void* x, const int64_t* y, int64_t B, int64_t C, float* lse,
                     float* rowloss, float* out, uint32_t* ticket) {
  AKKA_CHECK(B >= 1 && C >= 1 && B < (int64_t(1) << 27), "xent: bad shape");
  hipLaunchKernelGGL(xent_fwd_kernel, dim3(uint32_t(B)), dim3(kBlock), 0, s, static_cast<const bf16_t*>(x), y, B, C,
                     lse, rowloss, out, ticket);
  check_launch("xent_fwd");
}

void launch_xent_bwd(hipStream_t s, const void* x, const int64_t* y, int64_t B, int64_t C, const float* lse,
                     const float* stat, const float* go, void* gx) {
  AKKA_CHECK(B >= 1 && C >= 1, "xent: bad shape");
  hipLaunchKernelGGL(xent_bwd_kernel, dim3(uint32_t(B)), dim3(kBlock), 0, s, static_cast<const bf16_t*>(x), y, C, lse,
                     stat, go, static_cast<bf16_t*>(gx));
  check_launch("xent_bwd");
}

}  // namespace akka
