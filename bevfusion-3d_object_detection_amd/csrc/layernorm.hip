// layernorm.hip -- row-wise LayerNorm with the residual update in front of it, fwd + bwd (gfx950).
//
// The token stream of a transformer block is a row-major [M, C] matrix, and between two GEMMs a Swin block does, as separate
// library kernels over that stream: LayerNorm, cast, drop-path multiply, residual add (twice per block), and autograd mirrors
// each of them and adds a separate accumulation of the two gradient paths that meet in the stream.  One kernel family, three
// modes (the mode is which pointers are given):
//   norm        y = LN(x) * gamma + beta, mean_rstd
//   add + norm  s = x + scale[row / rows_per_sample] * branch (stored in x's dtype), y = LN(s) * gamma + beta, mean_rstd
//   add         s only
// and one backward: ds = dLN(dy) + dsum, dx = ds, dbranch = scale * ds, with dgamma / dbeta as one partial row per workgroup
// that a second small launch adds in a fixed order (no atomics: reruns are bit-identical).
//
// A row belongs to LPR consecutive lanes of one wave (4 .. 64, picked from C); a lane owns up to three 8-element chunks of it,
// chunk index = lane-in-row + i * LPR, so that the LPR lanes of a row read consecutive 16-byte (bf16) or 32-byte (f32) pieces.
// The whole row stays in registers: the mean, then the sum of squared differences (two passes over registers, one over memory),
// both reduced with xor shuffles inside the lane group.  All arithmetic is fp32; what is normalised is s AS STORED (rounded to
// its storage dtype), so the fused result equals the unfused one and the backward recomputes x_hat from the saved s.
#include "common.h"

namespace bfhip {
namespace {

constexpr int kNch = 3;            // 8-element chunks a lane can hold
constexpr int kMaxC = kNch * 8 * kWave;  // 1536
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxBlocks = 1024;   // grid cap (the backward's partial buffer has one row per block)

__device__ __forceinline__ float round_bf16(float f) { return bf16_to_f32(bf16_rne(f)); }

// 8 consecutive elements starting at element e of a bf16 (bf != 0) or f32 array; e is a multiple of 8 and the base 16-byte aligned.
// The dtype flag is uniform over the launch.
__device__ __forceinline__ void load8(const void *base, size_t e, int bf, float *o) {
  if (bf) {
    unpack8(*(const uint4 *)((const bf16_t *)base + e), o);
  } else {
    const float4 *p = (const float4 *)((const float *)base + e);
    const float4 a = p[0], b = p[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
}

__device__ __forceinline__ void store8(void *base, size_t e, int bf, const float *o) {
  if (bf) {
    *(uint4 *)((bf16_t *)base + e) = pack8(o);
  } else {
    float4 *p = (float4 *)((float *)base + e);
    p[0] = make_float4(o[0], o[1], o[2], o[3]);
    p[1] = make_float4(o[4], o[5], o[6], o[7]);
  }
}

// sum over the LPR lanes of a row; every lane of the group ends with the same bits (a + b == b + a at every level)
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

struct FwdArgs {
  const void *x, *branch;
  const float *scale, *gamma, *beta;
  void *s, *y;
  float *mean_rstd;
  int M, rps, C, x_bf, b_bf, y_bf;
  float eps;
};

template <int LPR>
__global__ __launch_bounds__(kBlock) void layernorm_fwd_kernel(const FwdArgs a) {
  constexpr int RPW = kWave / LPR, RPB = RPW * kWaves;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int gl = lane % LPR, grp = lane / LPR;
  const int nchunk = a.C >> 3;
  const bool norm = a.y != nullptr;
  const float fC = (float)a.C;
  bool ok[kNch];
  float gam[kNch][8], bet[kNch][8];
#pragma unroll
  for (int i = 0; i < kNch; ++i) {
    const int c = gl + i * LPR;
    ok[i] = c < nchunk;
    if (norm && ok[i]) {
      load8(a.gamma, (size_t)c * 8, 0, gam[i]);
      load8(a.beta, (size_t)c * 8, 0, bet[i]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) gam[i][j] = bet[i][j] = 0.f;
    }
  }
  for (long long row0 = (long long)blockIdx.x * RPB; row0 < a.M; row0 += (long long)gridDim.x * RPB) {
    const long long row = row0 + wave * RPW + grp;
    const bool act = row < a.M;  // a lane group is active or idle as a whole; idle groups compute on zeros and store nothing
    const size_t base = (size_t)(act ? row : 0) * a.C;
    float sc = 1.f;
    if (act && a.branch && a.scale) sc = a.scale[(int)row / a.rps];
    float v[kNch][8];
#pragma unroll
    for (int i = 0; i < kNch; ++i) {
      const size_t e = base + (size_t)(gl + i * LPR) * 8;
      if (act && ok[i]) {
        load8(a.x, e, a.x_bf, v[i]);
        if (a.branch) {
          float b[8];
          load8(a.branch, e, a.b_bf, b);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            v[i][j] = v[i][j] + sc * b[j];
            if (a.x_bf) v[i][j] = round_bf16(v[i][j]);
          }
          store8(a.s, e, a.x_bf, v[i]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
      }
    }
    if (!norm) continue;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kNch; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[i][j];
    const float mean = group_sum<LPR>(sum) / fC;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < kNch; ++i)
      if (ok[i]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float d = v[i][j] - mean;
          sq += d * d;
        }
      }
    const float rstd = 1.f / sqrtf(group_sum<LPR>(sq) / fC + a.eps);
#pragma unroll
    for (int i = 0; i < kNch; ++i)
      if (act && ok[i]) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * gam[i][j] + bet[i][j];
        store8(a.y, base + (size_t)(gl + i * LPR) * 8, a.y_bf, o);
      }
    if (act && gl == 0) *(float2 *)(a.mean_rstd + 2 * (size_t)row) = make_float2(mean, rstd);
  }
}

struct BwdArgs {
  const void *s;
  const float *mean_rstd, *gamma;
  const void *dy, *dsum;
  const float *scale;
  void *dx, *dbranch;
  float *partial;
  int M, rps, C, x_bf, b_bf, y_bf;
};

// AFF: also accumulate dgamma = sum_rows dy * x_hat and dbeta = sum_rows dy, and store this block's partial row [2][C]
template <int LPR, bool AFF>
__global__ __launch_bounds__(kBlock) void layernorm_bwd_kernel(const BwdArgs a) {
  constexpr int RPW = kWave / LPR, RPB = RPW * kWaves;
  __shared__ float red[AFF ? 2 * kMaxC : 1];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int gl = lane % LPR, grp = lane / LPR;
  const int nchunk = a.C >> 3;
  const bool norm = a.dy != nullptr;
  const float fC = (float)a.C;
  bool ok[kNch];
  float gam[kNch][8], dg[kNch][8], db[kNch][8];
#pragma unroll
  for (int i = 0; i < kNch; ++i) {
    const int c = gl + i * LPR;
    ok[i] = c < nchunk;
    if (norm && ok[i]) {
      load8(a.gamma, (size_t)c * 8, 0, gam[i]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) gam[i][j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) dg[i][j] = db[i][j] = 0.f;
  }
  for (long long row0 = (long long)blockIdx.x * RPB; row0 < a.M; row0 += (long long)gridDim.x * RPB) {
    const long long row = row0 + wave * RPW + grp;
    const bool act = row < a.M;
    const size_t base = (size_t)(act ? row : 0) * a.C;
    float ds[kNch][8];
#pragma unroll
    for (int i = 0; i < kNch; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) ds[i][j] = 0.f;
    if (norm) {
      float mean = 0.f, rstd = 0.f;
      if (act) {
        const float2 mr = *(const float2 *)(a.mean_rstd + 2 * (size_t)row);
        mean = mr.x;
        rstd = mr.y;
      }
      float xh[kNch][8];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < kNch; ++i) {
        if (act && ok[i]) {
          const size_t e = base + (size_t)(gl + i * LPR) * 8;
          float dyv[8];
          load8(a.s, e, a.x_bf, xh[i]);
          load8(a.dy, e, a.y_bf, dyv);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            xh[i][j] = (xh[i][j] - mean) * rstd;
            const float g = dyv[j] * gam[i][j];
            ds[i][j] = g;
            s1 += g;
            s2 += g * xh[i][j];
            if (AFF) {
              dg[i][j] += dyv[j] * xh[i][j];
              db[i][j] += dyv[j];
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) xh[i][j] = 0.f;
        }
      }
      const float m1 = group_sum<LPR>(s1) / fC, m2 = group_sum<LPR>(s2) / fC;
#pragma unroll
      for (int i = 0; i < kNch; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) ds[i][j] = rstd * (ds[i][j] - m1 - xh[i][j] * m2);
    }
    float sc = 1.f;
    if (act && a.dbranch && a.scale) sc = a.scale[(int)row / a.rps];
#pragma unroll
    for (int i = 0; i < kNch; ++i)
      if (act && ok[i]) {
        const size_t e = base + (size_t)(gl + i * LPR) * 8;
        if (a.dsum) {
          float t[8];
          load8(a.dsum, e, a.x_bf, t);
#pragma unroll
          for (int j = 0; j < 8; ++j) ds[i][j] = ds[i][j] + t[j];
        }
        if (a.dx) store8(a.dx, e, a.x_bf, ds[i]);
        if (a.dbranch) {
          float t[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) t[j] = sc * ds[i][j];
          store8(a.dbranch, e, a.b_bf, t);
        }
      }
  }
  if (AFF) {
    // the row groups of a wave own the same columns: add them with xor shuffles over the group index, then the four waves add in
    // turn through LDS (fixed order), then one coalesced store of this block's partial row
#pragma unroll
    for (int i = 0; i < kNch; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int o = LPR; o < kWave; o <<= 1) {
          dg[i][j] += __shfl_xor(dg[i][j], o, kWave);
          db[i][j] += __shfl_xor(db[i][j], o, kWave);
        }
    for (int w = 0; w < kWaves; ++w) {
      if (wave == w && grp == 0) {
#pragma unroll
        for (int i = 0; i < kNch; ++i)
          if (ok[i]) {
            const int c0 = (gl + i * LPR) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              red[c0 + j] = (w == 0 ? 0.f : red[c0 + j]) + dg[i][j];
              red[a.C + c0 + j] = (w == 0 ? 0.f : red[a.C + c0 + j]) + db[i][j];
            }
          }
      }
      __syncthreads();
    }
    float *dst = a.partial + (size_t)blockIdx.x * 2 * a.C;
    for (int i = threadIdx.x; i < 2 * a.C; i += kBlock) dst[i] = red[i];
  }
}

// out[col] = sum over the partial rows, in a fixed order: thread (cx, py) adds rows py, py + 4, ..; the four row lanes then add in turn
__global__ __launch_bounds__(kBlock) void layernorm_param_grad_kernel(const float *partial, int parts, int C, float *dgamma, float *dbeta) {
  __shared__ float red[kWaves][kWave];
  const int cx = threadIdx.x & (kWave - 1), py = threadIdx.x / kWave;
  const int col = blockIdx.x * kWave + cx;
  float acc = 0.f;
  if (col < 2 * C)
    for (int p = py; p < parts; p += kWaves) acc += partial[(size_t)p * 2 * C + col];
  red[py][cx] = acc;
  __syncthreads();
  if (py == 0 && col < 2 * C) {
    const float t = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
    if (col < C) dgamma[col] = t;
    else dbeta[col - C] = t;
  }
}

inline bool shape_ok(long long M, int C) { return M >= 1 && M <= 0x7fffffffll && C >= 8 && C <= kMaxC && C % 8 == 0; }
inline bool dtype_ok(int dt) { return dt == 0 || dt == 1; }

inline int lanes_per_row(int C) {
  int lpr = 4;
  while (lpr * kNch * 8 < C) lpr *= 2;
  return lpr;
}

// every block walks the same number of row slabs (the last one may be one short): no tail of a few blocks with one slab more
inline int grid_for(long long M, int C) {
  const int rpb = kWave / lanes_per_row(C) * kWaves;
  const long long slabs = (M + rpb - 1) / rpb;
  const long long iters = (slabs + kMaxBlocks - 1) / kMaxBlocks;
  return (int)((slabs + iters - 1) / iters);
}

#define BFHIP_LN_DISPATCH(LPR_VALUE, ...)                      \
  switch (LPR_VALUE) {                                         \
    case 4: { constexpr int LPR = 4; __VA_ARGS__; } break;          \
    case 8: { constexpr int LPR = 8; __VA_ARGS__; } break;          \
    case 16: { constexpr int LPR = 16; __VA_ARGS__; } break;        \
    case 32: { constexpr int LPR = 32; __VA_ARGS__; } break;        \
    default: { constexpr int LPR = 64; __VA_ARGS__; } break;        \
  }

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_layernorm_supported(long long M, int C, int x_dtype, int y_dtype) {
  return shape_ok(M, C) && dtype_ok(x_dtype) && dtype_ok(y_dtype) ? 1 : 0;
}

BFHIP_EXPORT int bfhip_layernorm_parts(long long M, int C) { return shape_ok(M, C) ? grid_for(M, C) : 0; }

BFHIP_EXPORT int bfhip_layernorm_fwd(const void *x, const void *branch, const float *scale, long long rows_per_sample,
                                     const float *gamma, const float *beta, long long M, int C, float eps, int x_dtype,
                                     int branch_dtype, int y_dtype, void *s, void *y, float *mean_rstd, void *stream) {
  BFHIP_REQUIRE(shape_ok(M, C) && dtype_ok(x_dtype) && dtype_ok(branch_dtype) && dtype_ok(y_dtype),
                "layernorm_fwd: unsupported M=%lld C=%d dtypes=%d/%d/%d", M, C, x_dtype, branch_dtype, y_dtype);
  BFHIP_REQUIRE(x && (branch || y), "layernorm_fwd: x and at least one of branch / y are required");
  BFHIP_REQUIRE((branch != nullptr) == (s != nullptr), "layernorm_fwd: s is the output of the add (given exactly when branch is)");
  BFHIP_REQUIRE(!y || (gamma && beta && mean_rstd), "layernorm_fwd: y needs gamma, beta and mean_rstd");
  BFHIP_REQUIRE(!scale || (branch && rows_per_sample >= 1 && rows_per_sample <= M), "layernorm_fwd: scale needs branch and 1 <= rows_per_sample <= M");
  BFHIP_REQUIRE(aligned16(x) && aligned16(branch) && aligned16(s) && aligned16(y) && aligned16(gamma) && aligned16(beta) &&
                    ((uintptr_t)mean_rstd % 8) == 0,
                "layernorm_fwd: tensors must be 16-byte aligned");
  FwdArgs a;
  a.x = x; a.branch = branch; a.scale = scale; a.gamma = gamma; a.beta = beta; a.s = s; a.y = y; a.mean_rstd = mean_rstd;
  a.M = (int)M; a.rps = scale ? (int)rows_per_sample : 1; a.C = C; a.x_bf = x_dtype; a.b_bf = branch_dtype; a.y_bf = y_dtype; a.eps = eps;
  const int grid = grid_for(M, C);
  BFHIP_LN_DISPATCH(lanes_per_row(C), hipLaunchKernelGGL(layernorm_fwd_kernel<LPR>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a));
  return check_launch("layernorm_fwd");
}

BFHIP_EXPORT int bfhip_layernorm_bwd(const void *s, const float *mean_rstd, const float *gamma, const void *dy, const void *dsum,
                                     const float *scale, long long rows_per_sample, long long M, int C, int x_dtype,
                                     int branch_dtype, int y_dtype, void *dx, void *dbranch, float *partial, int parts,
                                     float *dgamma, float *dbeta, void *stream) {
  BFHIP_REQUIRE(shape_ok(M, C) && dtype_ok(x_dtype) && dtype_ok(branch_dtype) && dtype_ok(y_dtype),
                "layernorm_bwd: unsupported M=%lld C=%d dtypes=%d/%d/%d", M, C, x_dtype, branch_dtype, y_dtype);
  BFHIP_REQUIRE(dy || dsum, "layernorm_bwd: at least one of dy / dsum is required");
  BFHIP_REQUIRE(!dy || (s && mean_rstd && gamma), "layernorm_bwd: dy needs s, mean_rstd and gamma");
  BFHIP_REQUIRE(dx || dbranch || partial, "layernorm_bwd: no output requested");
  BFHIP_REQUIRE(!scale || (rows_per_sample >= 1 && rows_per_sample <= M), "layernorm_bwd: scale needs 1 <= rows_per_sample <= M");
  BFHIP_REQUIRE((partial != nullptr) == (dgamma != nullptr) && (partial != nullptr) == (dbeta != nullptr),
                "layernorm_bwd: partial, dgamma and dbeta are given together or not at all");
  BFHIP_REQUIRE(!partial || dy, "layernorm_bwd: the parameter gradients need dy");
  const int grid = grid_for(M, C);
  BFHIP_REQUIRE(!partial || parts == grid, "layernorm_bwd: parts = %d, bfhip_layernorm_parts() says %d", parts, grid);
  BFHIP_REQUIRE(aligned16(s) && aligned16(gamma) && aligned16(dy) && aligned16(dsum) && aligned16(dx) && aligned16(dbranch) &&
                    ((uintptr_t)mean_rstd % 8) == 0,
                "layernorm_bwd: tensors must be 16-byte aligned");
  BwdArgs a;
  a.s = s; a.mean_rstd = mean_rstd; a.gamma = gamma; a.dy = dy; a.dsum = dsum; a.scale = scale; a.dx = dx; a.dbranch = dbranch;
  a.partial = partial;
  a.M = (int)M; a.rps = scale ? (int)rows_per_sample : 1; a.C = C; a.x_bf = x_dtype; a.b_bf = branch_dtype; a.y_bf = y_dtype;
  if (partial) {
    BFHIP_LN_DISPATCH(lanes_per_row(C), hipLaunchKernelGGL((layernorm_bwd_kernel<LPR, true>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a));
    int rc = check_launch("layernorm_bwd");
    if (rc != BFHIP_OK) return rc;
    hipLaunchKernelGGL(layernorm_param_grad_kernel, dim3(ceil_div(2 * C, kWave)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float *)partial, parts, C, dgamma, dbeta);
    return check_launch("layernorm_param_grad");
  }
  BFHIP_LN_DISPATCH(lanes_per_row(C), hipLaunchKernelGGL((layernorm_bwd_kernel<LPR, false>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, a));
  return check_launch("layernorm_bwd");
}
