// img_store.h -- what the kernels that write the image batch share (preprocess.hip, image_aug.hip): the run of kRun pixels a
// lane owns, its vector / element-wise loads and the 16-byte / element-wise stores of a run.
#pragma once
#include "common.h"

namespace bfhip {
namespace {

constexpr int kRun = 8;  // pixels per lane

// kRun source elements as fp32: one aligned vector access, or the first n element by element (the rest are never used)
__device__ __forceinline__ void load_run(const uint8_t *p, int n, float *o) {
  if (n == kRun && ((uintptr_t)p & 7) == 0) {
    const uint2 v = *(const uint2 *)p;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = (float)((v.x >> (8 * j)) & 0xffu);
      o[4 + j] = (float)((v.y >> (8 * j)) & 0xffu);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kRun; ++j) o[j] = j < n ? (float)p[j] : 0.f;
  }
}
__device__ __forceinline__ void load_run(const float *p, int n, float *o) {
  if (n == kRun && ((uintptr_t)p & 15) == 0) {
    const float4 a = *(const float4 *)p, b = *(const float4 *)(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < kRun; ++j) o[j] = j < n ? p[j] : 0.f;
  }
}

// N consecutive output elements: 16-byte stores (q is 16-byte aligned), or the first n element by element
template <int N>
__device__ __forceinline__ void store_run(float *q, const float *e, bool vec, int n) {
  if (vec) {
#pragma unroll
    for (int k = 0; k < N; k += 4) *(float4 *)(q + k) = make_float4(e[k], e[k + 1], e[k + 2], e[k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (k < n) q[k] = e[k];
  }
}
template <int N>
__device__ __forceinline__ void store_run(bf16_t *q, const float *e, bool vec, int n) {
  // NaN-canonical rounding: what torch gives for the same cast; pixels are finite, so the NaN rule never decides a bit here
  if (vec) {
#pragma unroll
    for (int k = 0; k < N; k += 8) {
      uint4 v;
      v.x = bf16_rne_nan_canonical(e[k]) | (bf16_rne_nan_canonical(e[k + 1]) << 16);
      v.y = bf16_rne_nan_canonical(e[k + 2]) | (bf16_rne_nan_canonical(e[k + 3]) << 16);
      v.z = bf16_rne_nan_canonical(e[k + 4]) | (bf16_rne_nan_canonical(e[k + 5]) << 16);
      v.w = bf16_rne_nan_canonical(e[k + 6]) | (bf16_rne_nan_canonical(e[k + 7]) << 16);
      *(uint4 *)(q + k) = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (k < n) q[k] = (bf16_t)bf16_rne_nan_canonical(e[k]);
  }
}

}  // namespace
}  // namespace bfhip
