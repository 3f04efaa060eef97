// gfx950 (MI355X / CDNA4) kernels of the chunk N-way sum.
//
// Hot spot K1 of SURVEY §2.3 (reference: the scalar JVM loop of
// ScatteredDataBuffer.reduce, SB:20-32).
//
// The sum is pure HBM streaming (nsrc reads + 1 write per element, no reuse),
// so the design goal is bytes-in-flight, not arithmetic:
//   * Vec: every lane issues 16-B loads for ALL sources of UNROLL vectors before
//     the first add (NSRC*UNROLL independent loads per lane), grid-stride over
//     the chunk with a grid capped at 8 blocks/CU x 256 CUs.  fp32 accumulate.
//   * Lds: each wave streams its own 1-KiB-per-source tiles through LDS with
//     global_load_lds_dwordx4 (LDS-DMA, no VGPR destination), double-buffered
//     with a counted vmcnt so tile t+1 is in flight while tile t is summed.
// Both are templated on the source count so the loads unroll completely.
// 64-lane waves throughout; blocks of 256 threads = 4 waves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include <cstdlib>
#include <cstring>

#include "elem.h"
#include "kernels.h"
#include "launch_util.h"

namespace akka {

namespace {

struct SrcTable {
  const void* p[kMaxReduceSrc];
  int32_t* fill;  // optional counts-row fill done by block 0 (saves a dispatch per round)
  int32_t fill_value;
  int32_t fill_n;
  int32_t head_n;  // elements below the aligned body (vector kernels, block 0)
};

__device__ __forceinline__ void do_fill(const SrcTable& t) {
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < t.fill_n; i += kBlock) t.fill[i] = t.fill_value;
}

// Misaligned head folded into a vector launch: the head_n elements just below
// the (16-B aligned) body pointers, summed by block 0 (saves a dispatch per
// chunk when the block offset is not a multiple of 16 B).
template <typename T, int NSRC>
__device__ __forceinline__ void do_head(const SrcTable& t, void* dst) {
  if (blockIdx.x == 0 && int(threadIdx.x) < t.head_n) {
    const int i = int(threadIdx.x) - t.head_n;
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < NSRC; ++s) acc += Elt<T>::to_f(static_cast<const T*>(t.p[s])[i]);
    static_cast<T*>(dst)[i] = Elt<T>::from_f(acc);
  }
}

// ---- Vec: loads straight to VGPRs ----------------------------------------------
// Load/store cache policy (measured by bench/stream_variants.hip, see
// profiles/README.md): nontemporal stores keep a streamed output from
// evicting the sources out of the 256 MiB Infinity Cache; nontemporal loads
// help once the sources do not fit there anyway.
enum VecPolicy : int { kNtl = 0, kNts = 1, kBoth = 2 };

template <typename T, int NSRC, int UNROLL, int POL>
__global__ __launch_bounds__(kBlock) void reduce_vec_kernel(SrcTable srcs, v4u* __restrict__ dst, int64_t nvec) {
  constexpr int E = Elt<T>::kPerVec;
  do_fill(srcs);
  do_head<T, NSRC>(srcs, dst);
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t base = int64_t(blockIdx.x) * kBlock + threadIdx.x; base < nvec; base += stride * UNROLL) {
    v4u v[UNROLL][NSRC];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t i = base + u * stride;
      if (i < nvec) {
#pragma unroll
        for (int s = 0; s < NSRC; ++s) {
          const v4u* src = static_cast<const v4u*>(srcs.p[s]) + i;
          v[u][s] = POL == kNts ? *src : __builtin_nontemporal_load(src);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t i = base + u * stride;
      if (i < nvec) {
        v4u o;
        if constexpr (NSRC == 1) {
          // one contributor: this body copies the vector, bit for bit (-0.0, NaN payloads).  The peeled head, the
          // scalar rest and the Lds kernel have no such case and add the source to +0.0 like any other count: the
          // same value, a NaN for a NaN, but -0.0 comes out as +0.0 and a payload is the adder's business
          o = v[u][0];
        } else {
          float acc[E];
#pragma unroll
          for (int e = 0; e < E; ++e) acc[e] = 0.f;
#pragma unroll
          for (int s = 0; s < NSRC; ++s) Elt<T>::add(acc, v[u][s]);
          o = Elt<T>::pack(acc);
        }
        if constexpr (POL == kNtl) dst[i] = o;
        else __builtin_nontemporal_store(o, dst + i);
      }
    }
  }
}

// ---- Lds: LDS-DMA staging, per-wave double buffer ----------------------------------
// Wave w of the block owns LDS [buf][src][w][64 lanes] x 16 B.  A tile is 64
// vectors (1 KiB) per source.  global_load_lds writes lane l's 16 B at
// wave_base + 16*l, i.e. exactly where lane l reads it back.
template <typename T, int NSRC>
__global__ __launch_bounds__(kBlock) void reduce_lds_kernel(SrcTable srcs, v4u* __restrict__ dst, int64_t nvec) {
  constexpr int E = Elt<T>::kPerVec;
  constexpr int kWaves = kBlock / 64;
  __shared__ v4u lds[2][NSRC][kWaves][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  do_fill(srcs);
  do_head<T, NSRC>(srcs, dst);
  const int64_t ntiles = nvec / 64;  // full wave tiles; the tail goes through VGPRs
  const int64_t wave_id = int64_t(blockIdx.x) * kWaves + wave;
  const int64_t wave_stride = int64_t(gridDim.x) * kWaves;

  auto issue = [&](int64_t tile, int buf) {
#pragma unroll
    for (int s = 0; s < NSRC; ++s) {
      const v4u* g = static_cast<const v4u*>(srcs.p[s]) + tile * 64 + lane;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                       (__attribute__((address_space(3))) void*)&lds[buf][s][wave][0], 16, 0, 0);
    }
  };

  int64_t t = wave_id;
  int buf = 0;
  if (t < ntiles) issue(t, 0);
  for (; t < ntiles; t += wave_stride) {
    const int64_t nt = t + wave_stride;
    if (nt < ntiles) {
      issue(nt, buf ^ 1);
      // NSRC loads of the next tile may stay in flight; the current tile's are retired
      // (loads retire in order; an interleaved store only makes the wait stricter).
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSRC) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
#pragma unroll
    for (int s = 0; s < NSRC; ++s) Elt<T>::add(acc, lds[buf][s][wave][lane]);
    dst[t * 64 + lane] = Elt<T>::pack(acc);
    // The reads of `buf` must land before tile t+2 re-targets it.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    buf ^= 1;
  }
  // Tail (< 64 vectors): first wave of the grid, through VGPRs.
  if (wave_id == 0) {
    const int64_t i = ntiles * 64 + lane;
    if (i < nvec) {
      float acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = 0.f;
#pragma unroll
      for (int s = 0; s < NSRC; ++s) Elt<T>::add(acc, static_cast<const v4u*>(srcs.p[s])[i]);
      dst[i] = Elt<T>::pack(acc);
    }
  }
}

// ---- Scalar: unaligned pointers / sub-vector tails --------------------------------

template <typename T>
__global__ __launch_bounds__(kBlock) void reduce_scalar_kernel(SrcTable srcs, int nsrc, T* __restrict__ dst,
                                                               int64_t n) {
  do_fill(srcs);
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    float acc = 0.f;
    for (int s = 0; s < nsrc; ++s) acc += Elt<T>::to_f(static_cast<const T*>(srcs.p[s])[i]);
    dst[i] = Elt<T>::from_f(acc);
  }
}

template <typename T, int NSRC, int POL, int UNROLL>
void launch_vec_u(hipStream_t s, const SrcTable& t, v4u* dst, int64_t nvec, int blocks_per_cu) {
  const int64_t cap = int64_t(kCUs) * blocks_per_cu;
  int64_t want = (nvec + int64_t(kBlock) * UNROLL - 1) / (int64_t(kBlock) * UNROLL);
  int grid = int(want < cap ? (want < 1 ? 1 : want) : cap);
  hipLaunchKernelGGL((reduce_vec_kernel<T, NSRC, UNROLL, POL>), dim3(grid), dim3(kBlock), 0, s, t, dst, nvec);
}

template <typename T, int NSRC, int POL>
void launch_vec_pol(hipStream_t s, const SrcTable& t, v4u* dst, int64_t nvec, int blocks_per_cu) {
  constexpr int U0 = NSRC <= 4 ? 4 : (NSRC <= 8 ? 2 : 1);
  // kBoth (big streams): 2 vectors per lane per source, but 4 for the
  // one-source pass (1 GiB bf16: 5.69 vs 5.53 TB/s at 2 blocks/CU, pass V)
  constexpr int UNROLL = POL == kBoth ? (NSRC == 1 ? 4 : (U0 < 2 ? U0 : 2)) : U0;
  if constexpr ((NSRC == 8 && POL == kNts && std::is_same<T, float>::value) || (NSRC == 1 && POL != kNtl)) {
    // experiments (bench/reduce_kernel_bw.py, bench/n1_bigcopy.py sweeps): loads in flight per lane
    static const int u = [] {
      const char* v = std::getenv("AKKA_VEC_UNROLL");
      return v ? std::atoi(v) : 0;
    }();
    if (u == 1) return launch_vec_u<T, NSRC, POL, 1>(s, t, dst, nvec, blocks_per_cu);
    if (u == 4) return launch_vec_u<T, NSRC, POL, 4>(s, t, dst, nvec, blocks_per_cu);
    if (u == 8) return launch_vec_u<T, NSRC, POL, 8>(s, t, dst, nvec, blocks_per_cu);
  }
  launch_vec_u<T, NSRC, POL, UNROLL>(s, t, dst, nvec, blocks_per_cu);
}

template <typename T, int NSRC>
void launch_vec_n(hipStream_t s, const SrcTable& t, v4u* dst, int64_t nvec, int pol, int blocks_per_cu) {
  if (pol == kNts) launch_vec_pol<T, NSRC, kNts>(s, t, dst, nvec, blocks_per_cu);
  else if (pol == kBoth) launch_vec_pol<T, NSRC, kBoth>(s, t, dst, nvec, blocks_per_cu);
  else launch_vec_pol<T, NSRC, kNtl>(s, t, dst, nvec, blocks_per_cu);
}

template <typename T, int NSRC>
void launch_lds_n(hipStream_t s, const SrcTable& t, v4u* dst, int64_t nvec) {
  constexpr int kWaves = kBlock / 64;
  int64_t tiles = nvec / 64;
  int64_t want = (tiles + kWaves * 2 - 1) / (kWaves * 2);  // >= 2 tiles per wave to pipeline
  int grid = int(want < kMaxGrid ? (want < 1 ? 1 : want) : kMaxGrid);
  hipLaunchKernelGGL((reduce_lds_kernel<T, NSRC>), dim3(grid), dim3(kBlock), 0, s, t, dst, nvec);
}

// Lds is instantiated for up to 8 sources; beyond that `lds` launches Vec.
template <typename T>
void launch_vec(hipStream_t s, const SrcTable& t, int nsrc, v4u* dst, int64_t nvec, bool lds, int pol,
                int blocks_per_cu) {
  const bool known = dispatch_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(nsrc, [&](auto k) {
    constexpr int K = decltype(k)::value;
    if constexpr (K <= 8) {
      if (lds) return launch_lds_n<T, K>(s, t, dst, nvec);
    }
    launch_vec_n<T, K>(s, t, dst, nvec, pol, blocks_per_cu);
  });
  if (!known) throw AkkaError("reduce: unsupported source count");
}

}  // namespace

ReduceImpl reduce_impl_from_name(const char* v) {
  if (!v) return ReduceImpl::Auto;
  if (!std::strcmp(v, "vec")) return ReduceImpl::Vec;
  if (!std::strcmp(v, "lds")) return ReduceImpl::Lds;
  if (!std::strcmp(v, "scalar")) return ReduceImpl::Scalar;
  if (!std::strcmp(v, "vec_nts")) return ReduceImpl::VecNts;
  if (!std::strcmp(v, "vec_ntl")) return ReduceImpl::VecNtl;
  if (!std::strcmp(v, "vec_both")) return ReduceImpl::VecBoth;
  return ReduceImpl::Auto;
}

ReduceImpl reduce_impl_from_env() { return reduce_impl_from_name(std::getenv("AKKA_REDUCE_IMPL")); }

const char* reduce_impl_name(ReduceImpl i) {
  switch (i) {
    case ReduceImpl::Vec:
      return "vec";
    case ReduceImpl::Lds:
      return "lds";
    case ReduceImpl::Scalar:
      return "scalar";
    case ReduceImpl::VecNts:
      return "vec_nts";
    case ReduceImpl::VecNtl:
      return "vec_ntl";
    case ReduceImpl::VecBoth:
      return "vec_both";
    default:
      return "auto";
  }
}

void launch_reduce(hipStream_t s, const ReduceSpec& spec, DType dt, ReduceImpl impl) {
  if (spec.n <= 0) return;
  AKKA_CHECK(spec.nsrc >= 1 && spec.nsrc <= kMaxReduceSrc, "reduce: bad source count");
  // Common misalignment (every pointer at the same offset mod 16 B, which the
  // data plane's layout guarantees): the body runs on 16-B vectors from the
  // first aligned element and block 0 also sums the few head elements.
  int32_t head = 0;
  ReduceSpec body = spec;
  if (impl != ReduceImpl::Scalar) {
    const uintptr_t mis = reinterpret_cast<uintptr_t>(spec.dst) & 15;
    bool same = mis != 0;
    for (int i = 0; i < spec.nsrc && same; ++i) same = (reinterpret_cast<uintptr_t>(spec.srcs[i]) & 15) == mis;
    const size_t es = dt == DType::F32 ? 4 : 2;
    const int64_t h = int64_t((16 - mis) / es);
    if (same && mis % es == 0 && spec.n > h + 64) {
      head = int32_t(h);
      body.dst = static_cast<char*>(spec.dst) + h * es;
      for (int i = 0; i < spec.nsrc; ++i) body.srcs[i] = static_cast<const char*>(spec.srcs[i]) + h * es;
      body.n = spec.n - h;
    }
  }
  const ReduceSpec& sp = body;
  SrcTable t{};
  bool aligned = (reinterpret_cast<uintptr_t>(sp.dst) & 15) == 0;
  for (int i = 0; i < sp.nsrc; ++i) {
    t.p[i] = sp.srcs[i];
    aligned &= (reinterpret_cast<uintptr_t>(sp.srcs[i]) & 15) == 0;
  }
  const int64_t per_vec = dt == DType::F32 ? 4 : 8;
  const int64_t nvec = aligned ? sp.n / per_vec : 0;
  const int64_t es_b = dt == DType::F32 ? 4 : 2;
  const int64_t rbytes = int64_t(sp.nsrc) * sp.n * es_b, wbytes = sp.n * es_b;
  if (impl == ReduceImpl::Auto) {
    // Measured (profiles/README.md): LDS-DMA staging wins while the working set
    // sits in the 256 MiB Infinity Cache (chunk-sized reduces inside a round,
    // data just landed from xGMI); direct 16-B loads win for larger streams.
    impl = (rbytes + wbytes <= (int64_t(96) << 20) && sp.nsrc <= 8) ? ReduceImpl::Lds : ReduceImpl::Vec;
  }
  // Vec load/store policy and grid (bench/stream_variants.hip sweep):
  //   sources fit the Infinity Cache      -> plain loads, NT stores, 16 blocks/CU (64 for one source)
  //   big stream with a big output        -> NT loads + NT stores, unroll 2 (4 for one source), 2 blocks/CU
  //   otherwise (many sources, <=256 MiB) -> NT loads, plain stores, 4 blocks/CU
  int pol = kNtl, bpc = 4;
  if (impl == ReduceImpl::Vec) {
    // one source (the N=1 round): a grid that covers the whole stream in one
    // pass, 76 vs 80-82 us per 256 MiB fp32 (profiles/r03/pass_ai)
    if (rbytes <= (int64_t(256) << 20)) pol = kNts, bpc = sp.nsrc == 1 ? 64 : 16;
    else if (wbytes >= (int64_t(512) << 20)) pol = kBoth, bpc = 2;  // 1 GiB bf16: 5.56 vs 5.11 TB/s at 4 (profiles/r03/pass_u, pass_v)
    else pol = kNtl, bpc = 4;
  } else if (impl == ReduceImpl::VecNts) {
    pol = kNts, bpc = 16;
  } else if (impl == ReduceImpl::VecBoth) {
    pol = kBoth, bpc = 2;
  } else if (impl == ReduceImpl::VecNtl) {
    pol = kNtl, bpc = 8;
  }
  bool filled = false;
  t.head_n = head;
  if (impl == ReduceImpl::Scalar) {
    // forced scalar path over everything
  } else if (nvec > 0) {
    const bool lds = impl == ReduceImpl::Lds;
    if (const char* g = std::getenv("AKKA_VEC_BPC")) bpc = std::max(1, std::atoi(g));  // experiments
    t.fill = sp.fill;
    t.fill_value = sp.fill_value;
    t.fill_n = sp.fill ? sp.fill_n : 0;
    filled = true;
    if (dt == DType::F32) launch_vec<float>(s, t, sp.nsrc, static_cast<v4u*>(sp.dst), nvec, lds, pol, bpc);
    else launch_vec<bf16_t>(s, t, sp.nsrc, static_cast<v4u*>(sp.dst), nvec, lds, pol, bpc);
    check_launch("reduce_vec");
  }
  const int64_t done = impl == ReduceImpl::Scalar ? 0 : nvec * per_vec;
  const int64_t rest = sp.n - done;
  if (rest > 0 || (!filled && sp.fill && sp.fill_n > 0)) {
    const size_t es = dt == DType::F32 ? 4 : 2;
    SrcTable tt{};
    if (!filled) {
      tt.fill = sp.fill;
      tt.fill_value = sp.fill_value;
      tt.fill_n = sp.fill ? sp.fill_n : 0;
    }
    for (int i = 0; i < sp.nsrc; ++i) tt.p[i] = static_cast<const char*>(sp.srcs[i]) + done * es;
    int64_t want = (rest + kBlock - 1) / kBlock;
    if (want < 1) want = 1;  // fill-only launch
    int grid = int(want < kMaxGrid ? want : kMaxGrid);
    if (dt == DType::F32) {
      hipLaunchKernelGGL(reduce_scalar_kernel<float>, dim3(grid), dim3(kBlock), 0, s, tt, sp.nsrc,
                         reinterpret_cast<float*>(static_cast<char*>(sp.dst) + done * es), rest);
    } else {
      hipLaunchKernelGGL(reduce_scalar_kernel<bf16_t>, dim3(grid), dim3(kBlock), 0, s, tt, sp.nsrc,
                         reinterpret_cast<bf16_t*>(static_cast<char*>(sp.dst) + done * es), rest);
    }
    check_launch("reduce_scalar");
  }
}

}  // namespace akka
