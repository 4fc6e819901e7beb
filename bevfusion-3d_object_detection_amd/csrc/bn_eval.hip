// bn_eval.hip -- BatchNorm on its RUNNING statistics (+ residual add) (+ ReLU) over a dense row-major [M, C] matrix, fwd + bwd
// (gfx950).  The matrix is a channels-last [N, C, H, W] activation (M = N*H*W) or a feature matrix [M, C].
//
// With fixed statistics the layer is a per-channel affine map, so both directions are one elementwise pass:
//   forward   y = act((x - mean) * a + beta [+ residual]),  a = gamma / sqrt(var + eps)       one launch, no workspace
//   backward  g = dy * [y > 0] (y is read only with ReLU);  dx = g * a;  dres = g             one launch
//             dgamma = sum_rows g * x_hat, dbeta = sum_rows g, x_hat = (x - mean) / sqrt(var + eps): one partial row
//             [2][C] per workgroup, added in a fixed order by a second small launch (no atomics: reruns are bit-identical)
// All arithmetic is fp32 with one rounding at the store.  The mean is subtracted FIRST: (x - mean) * a has no cancellation
// between a*x and a*mean, which a precomputed shift b = beta - mean*a would bring in.
//
// A thread owns one 16-byte channel vector (8 bf16 / 4 f32) for the whole launch, so its per-channel coefficients are derived
// once from the four parameter vectors and stay in registers.  The L = C / V vectors of a row belong to L consecutive threads
// and a workgroup covers R = 256 / L consecutive rows per iteration: one iteration reads R * L * 16 contiguous bytes.  A row
// of more than 256 vectors (up to 512: 2048 f32 channels) is cut into column tiles of 256 (blockIdx.y), R = 1.  The grid is
// capped at 2048 workgroups, which stride over the row groups.
//
// ROWS variants (bfhip_bn_eval_rows_*): the matrix is capacity-sized and only its first n = clamp(*rows_dev, 0, M) rows are
// active, n living on the device (static capacity mode of the sparse encoder).  Every workgroup reads n itself (one uniform
// load), walks the same row groups as the plain kernel over the capacity, and writes zeros to the rows [n, M) whatever the
// inputs hold there: their loads are still issued (in bounds) so the load pipeline is the plain kernel's, and their values are
// dropped by selects, never multiplied.  An active row gets the plain kernel's arithmetic, so its bits are the same.
#include "common.h"

namespace bfhip {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxVec = 512;     // vectors per row: one thread each, in column tiles of kBlock
constexpr int kMaxBlocks = 2048;
constexpr int kMinIters = 4;     // row groups per workgroup before the grid grows

// V consecutive f32 parameters starting at channel c (a multiple of V; the base is 16-byte aligned)
template <int V>
__device__ __forceinline__ void load_param(const float *p, int c, float *o) {
#pragma unroll
  for (int i = 0; i < V; i += 4) {
    const float4 v = *(const float4 *)(p + c + i);
    o[i] = v.x; o[i + 1] = v.y; o[i + 2] = v.z; o[i + 3] = v.w;
  }
}

struct Shape {
  long long M, groups;  // rows; row groups of R rows
  int C, L, Lb, R;      // channels; vectors per row; vectors per column tile (blockIdx.y); rows per workgroup iteration
};

// What a thread owns: channel vector cv (channels [col, col + V)) and row lane rl of every row group its workgroup walks.
struct Lane {
  int cv, rl;
  bool live;
  size_t col;
};
template <int V>
__device__ __forceinline__ Lane lane_of(const Shape &sh) {
  const int t = threadIdx.x;
  Lane ln;
  ln.cv = blockIdx.y * sh.Lb + t % sh.Lb;
  ln.rl = t / sh.Lb;
  ln.live = ln.rl < sh.R && ln.cv < sh.L;
  ln.col = (size_t)ln.cv * V;
  return ln;
}

// Walks the workgroup's row groups (grid stride) two at a time, then the odd one.  load(o, row) only issues the loads of the
// row at element offset o; use(o, row, keep) does the arithmetic and stores if keep.  Both loads go out before the first use.
// Only the LAST group can be short: a second row beyond M is loaded from the first row's address instead (a predicated load
// is a branch the compiler will not issue loads across) and its result is dropped.
template <typename Row, typename Load, typename Use>
__device__ __forceinline__ void walk_groups(const Shape &sh, const Lane &ln, Load load, Use use) {
  const long long step = gridDim.x;
  long long g = blockIdx.x;
  for (; g + step < sh.groups; g += 2 * step) {
    const long long r0 = g * sh.R + ln.rl, r1 = (g + step) * sh.R + ln.rl;  // r0 < M
    const bool ok1 = r1 < sh.M;
    const size_t o0 = (size_t)r0 * sh.C + ln.col, o1 = (size_t)(ok1 ? r1 : r0) * sh.C + ln.col;
    Row row[2];
    load(o0, row[0]);
    load(o1, row[1]);
    use(o0, row[0], true);
    use(o1, row[1], ok1);
  }
  if (g < sh.groups && g * sh.R + ln.rl < sh.M) {
    const size_t o0 = (size_t)(g * sh.R + ln.rl) * sh.C + ln.col;
    Row row;
    load(o0, row);
    use(o0, row, true);
  }
}

// first element offset beyond the active rows: offset o = row * C + col (col < C) is in an active row iff o < end
__device__ __forceinline__ size_t active_end(const int *rows_dev, const Shape &sh) {
  long long n = *rows_dev;  // uniform address: one scalar load per workgroup
  n = n < 0 ? 0 : (n > sh.M ? sh.M : n);
  return (size_t)n * sh.C;
}

template <typename T, bool RES, bool RELU, bool ROWS>
__global__ __launch_bounds__(kBlock) void bn_eval_fwd_kernel(const T *__restrict__ x, const T *__restrict__ res,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             const float *__restrict__ rmean, const float *__restrict__ rvar,
                                                             float eps, Shape sh, T *__restrict__ y,
                                                             const int *__restrict__ rows_dev) {
  constexpr int V = Vec16<T>::V;
  const Lane ln = lane_of<V>(sh);
  if (!ln.live) return;
  const size_t end = ROWS ? active_end(rows_dev, sh) : 0;
  float a[V], mean[V], b[V];
  {
    float var[V];
    load_param<V>(gamma, ln.cv * V, a);
    load_param<V>(rvar, ln.cv * V, var);
    load_param<V>(rmean, ln.cv * V, mean);
    load_param<V>(beta, ln.cv * V, b);
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] *= 1.f / sqrtf(var[j] + eps);
  }
  struct Row { float v[V], q[V]; };
  walk_groups<Row>(
      sh, ln,
      [=](size_t o, Row &w) {
        Vec16<T>::load(x + o, w.v);
        if (RES) Vec16<T>::load(res + o, w.q);
      },
      [&](size_t o, Row &w, bool keep) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          float r = fmaf(w.v[j] - mean[j], a[j], b[j]);
          if (RES) r += w.q[j];
          w.v[j] = (RELU && !(r > 0.f)) ? 0.f : r;
          if (ROWS && o >= end) w.v[j] = 0.f;
        }
        if (keep) Vec16<T>::store(y + o, w.v);
      });
}

// dx and dres are written where their pointer is given (uniform over the launch).  AFF: also accumulate this workgroup's
// partial row [2][C] = (sum g * x_hat, sum g) over its rows.
template <typename T, bool RELU, bool AFF, bool ROWS>
__global__ __launch_bounds__(kBlock) void bn_eval_bwd_kernel(const T *__restrict__ dy, const T *__restrict__ y,
                                                             const T *__restrict__ x, const float *__restrict__ gamma,
                                                             const float *__restrict__ rmean, const float *__restrict__ rvar,
                                                             float eps, Shape sh, T *__restrict__ dx, T *__restrict__ dres,
                                                             float *__restrict__ partial,
                                                             const int *__restrict__ rows_dev) {
  constexpr int V = Vec16<T>::V;
  __shared__ float sm[AFF ? 2 * kBlock * V : 1];
  const int t = threadIdx.x;
  const Lane ln = lane_of<V>(sh);
  float s0[V], s1[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s0[j] = s1[j] = 0.f;
  if (ln.live) {
    float a[V], mean[V], rstd[V];
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = mean[j] = rstd[j] = 0.f;
    if (dx || AFF) {
      load_param<V>(rvar, ln.cv * V, rstd);
#pragma unroll
      for (int j = 0; j < V; ++j) rstd[j] = 1.f / sqrtf(rstd[j] + eps);
    }
    if (dx) {
      load_param<V>(gamma, ln.cv * V, a);
#pragma unroll
      for (int j = 0; j < V; ++j) a[j] *= rstd[j];
    }
    if (AFF) load_param<V>(rmean, ln.cv * V, mean);
    const size_t end = ROWS ? active_end(rows_dev, sh) : 0;
    for (long long g = blockIdx.x; g < sh.groups; g += gridDim.x) {
      const long long r = g * sh.R + ln.rl;
      if (r >= sh.M) break;  // only the last group can be short
      const size_t o = (size_t)r * sh.C + ln.col;
      float gv[V], yv[V], xv[V];
      Vec16<T>::load(dy + o, gv);
      if (RELU) Vec16<T>::load(y + o, yv);
      if (AFF) Vec16<T>::load(x + o, xv);
      if (RELU) {
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (!(yv[j] > 0.f)) gv[j] = 0.f;
      }
      if (ROWS && o >= end) {  // a row beyond the count: g = 0 and x_hat = 0, so dx = dres = 0 and the sums get exact zeros
#pragma unroll
        for (int j = 0; j < V; ++j) {
          gv[j] = 0.f;
          if (AFF) xv[j] = mean[j];
        }
      }
      if (dres) Vec16<T>::store(dres + o, gv);
      if (AFF) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          s0[j] = fmaf(gv[j], (xv[j] - mean[j]) * rstd[j], s0[j]);
          s1[j] += gv[j];
        }
      }
      if (dx) {
#pragma unroll
        for (int j = 0; j < V; ++j) gv[j] *= a[j];
        Vec16<T>::store(dx + o, gv);
      }
    }
  }
  if (AFF) {
    // the R row lanes of a channel add in turn (fixed order), then one coalesced store of this column tile's piece of the
    // partial row.  Local channel cl (of the tile) of row lane rl lives at sm[rl * Lb * V + cl]
    float *m0 = sm, *m1 = sm + kBlock * V;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      m0[t * V + j] = s0[j];
      m1[t * V + j] = s1[j];
    }
    __syncthreads();
    const int nl = sh.Lb * V, c0 = blockIdx.y * nl;
    float *dst = partial + (size_t)blockIdx.x * 2 * sh.C + c0;
    for (int cl = t; cl < nl && c0 + cl < sh.C; cl += kBlock) {
      float p0 = 0.f, p1 = 0.f;
      for (int k = 0; k < sh.R; ++k) {
        p0 += m0[k * nl + cl];
        p1 += m1[k * nl + cl];
      }
      dst[cl] = p0;
      dst[sh.C + cl] = p1;
    }
  }
}

// dgb[col] = sum over the partial rows, in a fixed order: thread (cx, py) adds rows py, py + 4, ..; the four row lanes then add in turn
__global__ __launch_bounds__(kBlock) void bn_eval_param_grad_kernel(const float *__restrict__ partial, int parts, int C2,
                                                                    float *__restrict__ dgb) {
  constexpr int kRows = kBlock / kWave;
  __shared__ float red[kRows][kWave];
  const int cx = threadIdx.x & (kWave - 1), py = threadIdx.x / kWave;
  const int col = blockIdx.x * kWave + cx;
  float acc = 0.f;
  if (col < C2)
    for (int p = py; p < parts; p += kRows) acc += partial[(size_t)p * C2 + col];
  red[py][cx] = acc;
  __syncthreads();
  if (py == 0 && col < C2) dgb[col] = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
}

inline bool shape_ok(long long M, int C, int dtype) {
  if (dtype != 0 && dtype != 1) return false;
  const int V = 16 / elem_size(dtype);
  return M >= 1 && M <= 0x7fffffffll && C >= V && C % V == 0 && C / V <= kMaxVec;
}

inline Shape make_shape(long long M, int C, int dtype) {
  Shape sh;
  sh.M = M;
  sh.C = C;
  sh.L = C / (16 / elem_size(dtype));
  sh.Lb = sh.L < kBlock ? sh.L : kBlock;
  sh.R = kBlock / sh.Lb;
  sh.groups = (M + sh.R - 1) / sh.R;
  return sh;
}

inline int col_tiles(const Shape &sh) { return (sh.L + sh.Lb - 1) / sh.Lb; }

// every workgroup walks the same number of row groups (the last one may be one short), at least kMinIters where M allows
inline int grid_for(const Shape &sh, long long cap) {
  cap = cap / col_tiles(sh) > 0 ? cap / col_tiles(sh) : 1;
  long long blocks = (sh.groups + kMinIters - 1) / kMinIters;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const long long iters = (sh.groups + blocks - 1) / blocks;
  return (int)((sh.groups + iters - 1) / iters);
}

// workgroups of a backward that produces parameter gradients = rows of `partial`: the partial rows stay below a quarter of
// one activation tensor (the launch moves three or four of them)
inline int parts_for(const Shape &sh, int dtype) {
  long long cap = sh.M * elem_size(dtype) / 32;
  if (cap < 1) cap = 1;
  if (cap > kMaxBlocks) cap = kMaxBlocks;
  return grid_for(sh, cap);
}

template <typename T>
void launch_fwd(const void *x, const void *res, const float *gamma, const float *beta, const float *rmean, const float *rvar,
                float eps, const Shape &sh, int relu, void *y, const int *rows_dev, hipStream_t s) {
  const dim3 grid(grid_for(sh, kMaxBlocks), col_tiles(sh));
#define BFHIP_BN_EVAL_FWD(RES, RELU, ROWS)                                                                              \
  hipLaunchKernelGGL((bn_eval_fwd_kernel<T, RES, RELU, ROWS>), grid, dim3(kBlock), 0, s, (const T *)x, (const T *)res, \
                     gamma, beta, rmean, rvar, eps, sh, (T *)y, rows_dev)
#define BFHIP_BN_EVAL_FWD_ACT(RES, ROWS)                                                      \
  do {                                                                                        \
    if (relu) BFHIP_BN_EVAL_FWD(RES, true, ROWS); else BFHIP_BN_EVAL_FWD(RES, false, ROWS);   \
  } while (0)
  if (rows_dev) { if (res) BFHIP_BN_EVAL_FWD_ACT(true, true); else BFHIP_BN_EVAL_FWD_ACT(false, true); }
  else { if (res) BFHIP_BN_EVAL_FWD_ACT(true, false); else BFHIP_BN_EVAL_FWD_ACT(false, false); }
#undef BFHIP_BN_EVAL_FWD_ACT
#undef BFHIP_BN_EVAL_FWD
}

template <typename T>
void launch_bwd(const void *dy, const void *y, const void *x, const float *gamma, const float *rmean, const float *rvar,
                float eps, const Shape &sh, int relu, void *dx, void *dres, float *partial, int grid_x, const int *rows_dev,
                hipStream_t s) {
  const dim3 grid(grid_x, col_tiles(sh));
#define BFHIP_BN_EVAL_BWD(RELU, AFF, ROWS)                                                                            \
  hipLaunchKernelGGL((bn_eval_bwd_kernel<T, RELU, AFF, ROWS>), grid, dim3(kBlock), 0, s, (const T *)dy, (const T *)y,  \
                     (const T *)x, gamma, rmean, rvar, eps, sh, (T *)dx, (T *)dres, partial, rows_dev)
#define BFHIP_BN_EVAL_BWD_ACT(AFF, ROWS)                                                      \
  do {                                                                                        \
    if (relu) BFHIP_BN_EVAL_BWD(true, AFF, ROWS); else BFHIP_BN_EVAL_BWD(false, AFF, ROWS);   \
  } while (0)
  if (rows_dev) { if (partial) BFHIP_BN_EVAL_BWD_ACT(true, true); else BFHIP_BN_EVAL_BWD_ACT(false, true); }
  else { if (partial) BFHIP_BN_EVAL_BWD_ACT(true, false); else BFHIP_BN_EVAL_BWD_ACT(false, false); }
#undef BFHIP_BN_EVAL_BWD_ACT
#undef BFHIP_BN_EVAL_BWD
}

// the two directions' host bodies; rows_dev = nullptr: every row is active
int run_fwd(const char *what, const void *x, const void *residual, const float *gamma, const float *beta,
            const float *running_mean, const float *running_var, long long M, int C, int dtype, float eps, int relu, void *y,
            const int *rows_dev, hipStream_t stream) {
  BFHIP_REQUIRE(shape_ok(M, C, dtype), "%s: unsupported M=%lld C=%d dtype=%d", what, M, C, dtype);
  BFHIP_REQUIRE(x && y && gamma && beta && running_mean && running_var,
                "%s: x, y, gamma, beta and the running statistics are required", what);
  BFHIP_REQUIRE(aligned16(x) && aligned16(residual) && aligned16(y) && aligned16(gamma) && aligned16(beta) &&
                    aligned16(running_mean) && aligned16(running_var),
                "%s: tensors must be 16-byte aligned", what);
  const Shape sh = make_shape(M, C, dtype);
  if (dtype == 1)
    launch_fwd<bf16_t>(x, residual, gamma, beta, running_mean, running_var, eps, sh, relu, y, rows_dev, stream);
  else
    launch_fwd<float>(x, residual, gamma, beta, running_mean, running_var, eps, sh, relu, y, rows_dev, stream);
  return check_launch(what);
}

int run_bwd(const char *what, const void *dy, const void *y, const void *x, const float *gamma, const float *running_mean,
            const float *running_var, long long M, int C, int dtype, float eps, int relu, void *dx, void *dres, float *partial,
            float *dgb, const int *rows_dev, hipStream_t stream) {
  BFHIP_REQUIRE(shape_ok(M, C, dtype), "%s: unsupported M=%lld C=%d dtype=%d", what, M, C, dtype);
  BFHIP_REQUIRE(dy, "%s: dy is required", what);
  BFHIP_REQUIRE(!relu || y, "%s: the ReLU mask needs y", what);
  BFHIP_REQUIRE((x != nullptr) == (partial != nullptr) && (x != nullptr) == (dgb != nullptr),
                "%s: x, partial and dgb are given together or not at all", what);
  BFHIP_REQUIRE(dx || dres || partial, "%s: no output requested", what);
  BFHIP_REQUIRE(!dx || (gamma && running_var), "%s: dx needs gamma and running_var", what);
  BFHIP_REQUIRE(!partial || (running_mean && running_var), "%s: the parameter gradients need the running statistics", what);
  BFHIP_REQUIRE(aligned16(dy) && aligned16(y) && aligned16(x) && aligned16(dx) && aligned16(dres) && aligned16(gamma) &&
                    aligned16(running_mean) && aligned16(running_var) && aligned16(partial) && aligned16(dgb),
                "%s: tensors must be 16-byte aligned", what);
  const Shape sh = make_shape(M, C, dtype);
  const int grid = partial ? parts_for(sh, dtype) : grid_for(sh, kMaxBlocks);
  if (dtype == 1)
    launch_bwd<bf16_t>(dy, relu ? y : nullptr, x, gamma, running_mean, running_var, eps, sh, relu, dx, dres, partial, grid,
                       rows_dev, stream);
  else
    launch_bwd<float>(dy, relu ? y : nullptr, x, gamma, running_mean, running_var, eps, sh, relu, dx, dres, partial, grid,
                      rows_dev, stream);
  int rc = check_launch(what);
  if (rc != BFHIP_OK || !partial) return rc;
  hipLaunchKernelGGL(bn_eval_param_grad_kernel, dim3(ceil_div(2 * C, kWave)), dim3(kBlock), 0, stream, (const float *)partial,
                     grid, 2 * C, dgb);
  return check_launch("bn_eval_param_grad");
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_bn_eval_supported(long long M, int C, int dtype) { return shape_ok(M, C, dtype) ? 1 : 0; }

BFHIP_EXPORT int bfhip_bn_eval_parts(long long M, int C, int dtype) {
  return shape_ok(M, C, dtype) ? parts_for(make_shape(M, C, dtype), dtype) : 0;
}

BFHIP_EXPORT int bfhip_bn_eval_fwd(const void *x, const void *residual, const float *gamma, const float *beta,
                                   const float *running_mean, const float *running_var, long long M, int C, int dtype, float eps,
                                   int relu, void *y, void *stream) {
  return run_fwd("bn_eval_fwd", x, residual, gamma, beta, running_mean, running_var, M, C, dtype, eps, relu, y, nullptr,
                 (hipStream_t)stream);
}

BFHIP_EXPORT int bfhip_bn_eval_bwd(const void *dy, const void *y, const void *x, const float *gamma, const float *running_mean,
                                   const float *running_var, long long M, int C, int dtype, float eps, int relu, void *dx,
                                   void *dres, float *partial, float *dgb, void *stream) {
  return run_bwd("bn_eval_bwd", dy, y, x, gamma, running_mean, running_var, M, C, dtype, eps, relu, dx, dres, partial, dgb,
                 nullptr, (hipStream_t)stream);
}

BFHIP_EXPORT int bfhip_bn_eval_rows_fwd(const void *x, const void *residual, const float *gamma, const float *beta,
                                        const float *running_mean, const float *running_var, long long M, int C, int dtype,
                                        float eps, int relu, void *y, const int *rows_dev, void *stream) {
  BFHIP_REQUIRE(rows_dev, "bn_eval_rows_fwd: rows_dev is required");
  return run_fwd("bn_eval_rows_fwd", x, residual, gamma, beta, running_mean, running_var, M, C, dtype, eps, relu, y, rows_dev,
                 (hipStream_t)stream);
}

BFHIP_EXPORT int bfhip_bn_eval_rows_bwd(const void *dy, const void *y, const void *x, const float *gamma,
                                        const float *running_mean, const float *running_var, long long M, int C, int dtype,
                                        float eps, int relu, void *dx, void *dres, float *partial, float *dgb,
                                        const int *rows_dev, void *stream) {
  BFHIP_REQUIRE(rows_dev, "bn_eval_rows_bwd: rows_dev is required");
  return run_bwd("bn_eval_rows_bwd", dy, y, x, gamma, running_mean, running_var, M, C, dtype, eps, relu, dx, dres, partial, dgb,
                 rows_dev, (hipStream_t)stream);
}
