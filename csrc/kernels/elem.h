// The element codec of every kernel unit: one 16-byte vector type and, per
// element type, the fp32 accumulate of a vector, the pack of the accumulators
// and the scalar conversions.  Sums accumulate in fp32; bf16 is rounded in one
// place (Elt<bf16_t>::from_f), so a sum is the same bits whichever kernel made
// it.  Only to be included by .hip translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace akka {

// 16 bytes per lane per access (ext-vector: the nontemporal and raw-buffer
// builtins take it as it is).
using v4u = unsigned int __attribute__((ext_vector_type(4)));
// Storage of one bf16 element.
using bf16_t = uint16_t;

template <typename T>
struct Elt;

template <>
struct Elt<float> {
  static constexpr int kPerVec = 4;
  __device__ __forceinline__ static float to_f(float v) { return v; }
  __device__ __forceinline__ static float from_f(float v) { return v; }
  __device__ __forceinline__ static void add(float (&acc)[4], const v4u& v) {
    acc[0] += __uint_as_float(v.x);
    acc[1] += __uint_as_float(v.y);
    acc[2] += __uint_as_float(v.z);
    acc[3] += __uint_as_float(v.w);
  }
  __device__ __forceinline__ static v4u pack(const float (&acc)[4]) {
    return v4u{__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]), __float_as_uint(acc[3])};
  }
  __device__ __forceinline__ static float load1(const char* p) { return *reinterpret_cast<const float*>(p); }
  __device__ __forceinline__ static void store1(char* p, float v) { *reinterpret_cast<float*>(p) = v; }
};

template <>
struct Elt<bf16_t> {
  static constexpr int kPerVec = 8;
  __device__ __forceinline__ static float to_f(bf16_t v) { return __uint_as_float(uint32_t(v) << 16); }
  // The plain cast lowers to v_cvt_pk_bf16_f32 on gfx950 (RNE, NaN-preserving).
  __device__ __forceinline__ static bf16_t from_f(float v) {
    return __builtin_bit_cast(bf16_t, static_cast<__bf16>(v));
  }
  __device__ __forceinline__ static void add(float (&acc)[8], const v4u& v) {
    acc[0] += __uint_as_float(v.x << 16);
    acc[1] += __uint_as_float(v.x & 0xffff0000u);
    acc[2] += __uint_as_float(v.y << 16);
    acc[3] += __uint_as_float(v.y & 0xffff0000u);
    acc[4] += __uint_as_float(v.z << 16);
    acc[5] += __uint_as_float(v.z & 0xffff0000u);
    acc[6] += __uint_as_float(v.w << 16);
    acc[7] += __uint_as_float(v.w & 0xffff0000u);
  }
  __device__ __forceinline__ static uint32_t pack2(float lo, float hi) {
    return uint32_t(from_f(lo)) | (uint32_t(from_f(hi)) << 16);
  }
  __device__ __forceinline__ static v4u pack(const float (&acc)[8]) {
    return v4u{pack2(acc[0], acc[1]), pack2(acc[2], acc[3]), pack2(acc[4], acc[5]), pack2(acc[6], acc[7])};
  }
  __device__ __forceinline__ static float load1(const char* p) { return to_f(*reinterpret_cast<const bf16_t*>(p)); }
  __device__ __forceinline__ static void store1(char* p, float v) { *reinterpret_cast<bf16_t*>(p) = from_f(v); }
};

}  // namespace akka
