// The element codec of every kernel unit: one 16-byte vector type and, per
// element type, the fp32 accumulate of a vector, the pack of the accumulators
// and the scalar conversions.  Sums accumulate in fp32; bf16 is rounded in one
// place (Elt<bf16_t>::from_f), so a sum is the same bits whichever kernel made
// it; the one other rounding is sr_bf16 below, the stochastic one of the
// optimizer's bf16 moments and bf16 parameters.  Only to be included by .hip translation units.
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

// Element q of a unit's vectors widened to fp32, bit for bit (Elt<T>::add onto
// a zero would turn -0 into +0).  q is a constant after unrolling.
template <typename T>
__device__ __forceinline__ float unit_elem(const v4u* u, int q) {
  if constexpr (Elt<T>::kPerVec == 8) {
    const uint32_t w = u[q >> 3][(q >> 1) & 3];
    return __uint_as_float((q & 1) ? (w & 0xffff0000u) : (w << 16));
  } else {
    return __uint_as_float(u[q >> 2][q & 3]);
  }
}

// Stochastic rounding of fp32 to bf16 with 16 random bits r: the bits below
// the bf16 mantissa plus r carry into it with probability (those bits) / 2^16,
// so the expectation of the result is x.  A finite x that rounds up past the
// largest bf16 becomes inf, as under round-to-nearest.  The add would carry a
// NaN's payload into the exponent and the sign, so a non-finite x takes the
// NaN-preserving codec above.  (The definition of r: optim.hip.)
__device__ __forceinline__ bf16_t sr_bf16(float x, uint32_t r) {
  const uint32_t b = __float_as_uint(x);
  if ((b & 0x7f800000u) == 0x7f800000u) return Elt<bf16_t>::from_f(x);
  return bf16_t((b + (r & 0xffffu)) >> 16);
}

// The 32-bit mixer of the rounding bits (two multiplies, three xor-shifts; a bijection).
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

}  // namespace akka
