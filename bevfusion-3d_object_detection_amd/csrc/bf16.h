// bf16.h -- the only place that knows what a bf16 is: the storage type, the two conversions and the 16-byte vector access.
#pragma once
#include <hip/hip_runtime.h>

namespace bfhip {

typedef unsigned short bf16_t;

__device__ __forceinline__ float bf16_to_f32(unsigned bits) { return __uint_as_float(bits << 16); }

// fp32 -> bf16, round to nearest even; a NaN keeps its payload and gets the quiet bit
__device__ __forceinline__ unsigned bf16_rne(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// ... with every NaN mapped to 0x7fc0, as torch's own conversion does
__device__ __forceinline__ unsigned bf16_rne_nan_canonical(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// 8 consecutive bf16 (one 16-byte vector) <-> 8 floats
__device__ __forceinline__ void unpack8(uint4 v, float *o) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    o[2 * i] = __uint_as_float(w[i] << 16);
    o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 pack8(const float *o) {
  uint4 v;
  v.x = bf16_rne(o[0]) | (bf16_rne(o[1]) << 16);
  v.y = bf16_rne(o[2]) | (bf16_rne(o[3]) << 16);
  v.z = bf16_rne(o[4]) | (bf16_rne(o[5]) << 16);
  v.w = bf16_rne(o[6]) | (bf16_rne(o[7]) << 16);
  return v;
}

// one 16-byte vector of T as V floats (p is 16-byte aligned)
template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ void load(const float *p, float *o) {
    const float4 v = *(const float4 *)p;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  static __device__ __forceinline__ void store(float *p, const float *o) { *(float4 *)p = make_float4(o[0], o[1], o[2], o[3]); }
};
template <> struct Vec16<bf16_t> {
  static constexpr int V = 8;
  static __device__ __forceinline__ void load(const bf16_t *p, float *o) { unpack8(*(const uint4 *)p, o); }
  static __device__ __forceinline__ void store(bf16_t *p, const float *o) { *(uint4 *)p = pack8(o); }
};

}  // namespace bfhip
