// points_tile.h -- what the two point units (points_aug.hip, points_in_boxes.hip) share on the device: the row tile and the
// plane expression of the box test.
#pragma once
#include <hip/hip_runtime.h>

namespace bfhip {

constexpr int kPlaneFloats = 24;  // a box: 6 planes x (n0, n1, n2, d)

// the block's rows into LDS: rows [first, first + rows) of src, C floats each (12-32 B, not 16-byte aligned in general), as one
// contiguous run of dwords -- consecutive lanes load consecutive dwords.  Block = the workgroup's threads.
template <int Block>
__device__ __forceinline__ void stage_rows(const float *__restrict__ src, long long first, int rows, int C, float *tile) {
  const float *p = src + first * C;
  const int nd = rows * C;
  for (int d = threadIdx.x; d < nd; d += Block) tile[d] = p[d];
}

// ((x n0 + y n1) + z n2) + d of one plane pl = (n0, n1, n2, d), every product and sum a separate float32 operation.  The
// comparison stays with the caller: the units differ in what a NaN does.
__device__ __forceinline__ float plane_sign(const float *pl, float x, float y, float z) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, pl[0]), __fmul_rn(y, pl[1])), __fmul_rn(z, pl[2])), pl[3]);
}

}  // namespace bfhip
