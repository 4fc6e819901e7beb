// visualize.hip -- predicted boxes drawn on the camera frames and on a bird's-eye canvas (gfx950), as bevfusion_amd/visualize.py
// defines them bit for bit (the reference's tools/visualize/visualize_bboxes_bevfusion.py and visualize_bev.py go through
// matplotlib on the host).
//
//   1. vis_setup_kernel: one thread per (view, box, edge).  Corners from the box table (x, y, z, dx, dy, dz, cos, sin: the host
//      makes the cosine and sine), camera transform, near-plane clip, projection, all float32 with every product, sum and quotient
//      one rounded operation (__fmul_rn / __fadd_rn / __fdiv_rn: nothing contracts them); then 1/16-pixel fixed point (round to
//      nearest even) and the guard-rectangle clip in int64.  Out: one 32-byte record per edge -- the ends, the thickness, the box
//      index and the box of pixels the edge can cover, empty for a dropped edge.  The BEV mode maps footprint corners to the canvas.
//   2. vis_composite_kernel<S>: one workgroup of 256 threads per 32 x 8 tile of the OUTPUT mosaic.  The view's records go through
//      LDS in chunks of 256: each wave tests the pixel boxes of 64 records (a dense 8-byte side array: every tile walks all of its
//      view's records, and that walk is the kernel's traffic) against the tile's source rectangle, keeps the survivors in its own LDS list
//      by ballot and prefix popcount, and every lane then evaluates all survivors for its S x S source pixels with selects only
//      (no lane leaves the loop early, so the loop stays wave-uniform).  The highest covering box index gives the colour; the lane
//      reads the source pixel where nothing covers it, averages its S x S block and writes the mosaic cell.  Tiling, grid
//      placement, black cells and the downscale live in this launch: the camera mosaic is two launches for any number of views.
//      LDS: 4 x 64 records x 32 B = 8 KiB of lists per workgroup (12 KiB as compiled), so LDS never limits occupancy (160 KiB per
//      CU); the int64 coverage test is what holds the registers (30 for S = 1 to 101 for S = 4: 8 to 4 waves per SIMD).
//   3. vis_points_kernel: one thread per point stores a white square.  Every writer stores the same value, so the order cannot
//      matter and no atomic is needed.
// No atomics, no allocation, no host read: the same bytes on every run.
#include "common.h"

namespace bfhip {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kTileW = 32, kTileH = 8;
static_assert(kTileW * kTileH == kBlock, "one lane per output pixel of a tile");
constexpr int kChunk = kBlock;       // records per LDS pass: one per thread
constexpr int kMaxDim = 8192;        // pixels a side: 16 * kMaxDim + kGuard < 2^18
constexpr int kMaxT = 2048;          // thickness, 1/16 pixel: R^2 d.d < 2^22 * 2^39
constexpr int kMaxScale = 4;
constexpr long long kGuard = 2048;   // 1/16 pixel: > kMaxT / 2, so what the clip removes covers no pixel of the frame
constexpr float kFixLimit = 536870912.f;      // 2^29: |X|, |Y| below it make every product of the guard clip < 2^60
constexpr long long kCrossLimit = 1ll << 31;  // |cross| at or above it: cross^2 >= 2^62 > R^2 d.d, not covered

struct Seg {
  int x0, y0, x1, y1;  // ends, 1/16 pixel, inside the guard rectangle
  int lo, hi;          // col0 | row0 << 16, col1 | row1 << 16: the pixels the edge can cover; lo > hi fields: none
  int box, t;
};
static_assert(sizeof(Seg) == 32, "two 16-byte loads per record");
constexpr int kEmptyLo = 1 | (1 << 16);

// rounded num / den, halves up; den != 0, |2 num + den| < 2^62
__device__ __forceinline__ long long rdiv(long long num, long long den) {
  if (den < 0) num = -num, den = -den;
  const long long a = 2 * num + den, b = 2 * den;
  long long q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

// clip along a to [lo, hi], b interpolated: end 0 against lo, hi, then end 1 (the order is part of the specification)
__device__ __forceinline__ bool clip_axis(long long &a0, long long &b0, long long &a1, long long &b1, long long lo, long long hi) {
  if ((a0 < lo && a1 < lo) || (a0 > hi && a1 > hi)) return false;
  if (a0 < lo) { b0 += rdiv((b1 - b0) * (lo - a0), a1 - a0); a0 = lo; }
  if (a0 > hi) { b0 += rdiv((b1 - b0) * (hi - a0), a1 - a0); a0 = hi; }
  if (a1 < lo) { b1 += rdiv((b0 - b1) * (lo - a1), a0 - a1); a1 = lo; }
  if (a1 > hi) { b1 += rdiv((b0 - b1) * (hi - a1), a0 - a1); a1 = hi; }
  return true;
}

__device__ __forceinline__ long long lmin(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long lmax(long long a, long long b) { return a > b ? a : b; }

__device__ __forceinline__ Seg make_record(bool keep, float u0, float v0, float u1, float v1, int box, int t, int H, int W) {
  Seg s = {0, 0, 0, 0, kEmptyLo, 0, box, t};
  const float q0 = rintf(__fmul_rn(u0, 16.f)), q1 = rintf(__fmul_rn(v0, 16.f));
  const float q2 = rintf(__fmul_rn(u1, 16.f)), q3 = rintf(__fmul_rn(v1, 16.f));
  keep = keep && fabsf(q0) < kFixLimit && fabsf(q1) < kFixLimit && fabsf(q2) < kFixLimit && fabsf(q3) < kFixLimit;  // NaN fails
  if (!keep) return s;
  long long x0 = (long long)q0, y0 = (long long)q1, x1 = (long long)q2, y1 = (long long)q3;
  if (!clip_axis(x0, y0, x1, y1, -kGuard, 16ll * W + kGuard)) return s;
  if (!clip_axis(y0, x0, y1, x1, -kGuard, 16ll * H + kGuard)) return s;
  // pixel col's centre, 32 col + 16 in 1/32 pixel, within t of [2 xmin, 2 xmax]; >> 5 is the floor
  const long long c0 = lmax(-((-(2 * lmin(x0, x1) - t - 16)) >> 5), 0), c1 = lmin((2 * lmax(x0, x1) + t - 16) >> 5, W - 1);
  const long long r0 = lmax(-((-(2 * lmin(y0, y1) - t - 16)) >> 5), 0), r1 = lmin((2 * lmax(y0, y1) + t - 16) >> 5, H - 1);
  if (c0 > c1 || r0 > r1) return s;
  s.x0 = (int)x0, s.y0 = (int)y0, s.x1 = (int)x1, s.y1 = (int)y1;
  s.lo = (int)(c0 | (r0 << 16)), s.hi = (int)(c1 | (r1 << 16));
  return s;
}

// ((m0 p0 + m1 p1) + m2 p2) + m3
__device__ __forceinline__ float affine_row(const float *m, float p0, float p1, float p2) {
  return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], p0), __fmul_rn(m[1], p1)), __fmul_rn(m[2], p2)), m[3]);
}

__device__ __forceinline__ bool finite8(const float *b) {
  bool ok = true;
  for (int i = 0; i < 8; ++i) ok = ok && isfinite(b[i]);
  return ok;
}

// corner k of the reference's order: (ix, iy, iz) = (k >> 2, (k >> 1) & 1, (k ^ (k >> 1)) & 1), minus (0.5, 0.5, 0)
__device__ __forceinline__ void box_corner(const float *b, int k, float &px, float &py, float &pz) {
  const float ux = (k >> 2) ? 0.5f : -0.5f, uy = ((k >> 1) & 1) ? 0.5f : -0.5f, uz = ((k ^ (k >> 1)) & 1) ? 1.f : 0.f;
  const float lx = __fmul_rn(b[3], ux), ly = __fmul_rn(b[4], uy), lz = __fmul_rn(b[5], uz);
  const float c = b[6], s = b[7];
  px = __fadd_rn(__fadd_rn(__fmul_rn(lx, c), __fmul_rn(ly, -s)), b[0]);
  py = __fadd_rn(__fadd_rn(__fmul_rn(lx, s), __fmul_rn(ly, c)), b[1]);
  pz = __fadd_rn(lz, b[2]);
}

__constant__ int kEdgeA[12] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3};
__constant__ int kEdgeB[12] = {1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7};
__constant__ int kFootA[4] = {0, 3, 7, 4};
__constant__ int kFootB[4] = {3, 7, 4, 0};

// bev != 0: footprint edges on the canvas, u = (x - ox) ppm, v = (oy - y) ppm (oy the UPPER y limit)
__global__ __launch_bounds__(kBlock) void vis_setup_kernel(const float *__restrict__ table, int n, const float *__restrict__ L,
                                                           const float *__restrict__ K, int views, int bev, float near, float ox,
                                                           float oy, float ppm, int t, int H, int W, Seg *__restrict__ rec,
                                                           int2 *__restrict__ boxes_px) {
  const int E = bev ? 4 : 12;
  const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (long long)views * n * E) return;
  const int e = (int)(idx % E), box = (int)((idx / E) % n), view = (int)(idx / ((long long)E * n));
  float b[8];
  for (int i = 0; i < 8; ++i) b[i] = table[(size_t)box * 8 + i];
  bool keep = finite8(b);
  float ax, ay, az, bx, by, bz;
  box_corner(b, bev ? kFootA[e] : kEdgeA[e], ax, ay, az);
  box_corner(b, bev ? kFootB[e] : kEdgeB[e], bx, by, bz);
  float u0, v0, u1, v1;
  if (bev) {
    u0 = __fmul_rn(__fsub_rn(ax, ox), ppm), v0 = __fmul_rn(__fsub_rn(oy, ay), ppm);
    u1 = __fmul_rn(__fsub_rn(bx, ox), ppm), v1 = __fmul_rn(__fsub_rn(oy, by), ppm);
  } else {
    const float *Lm = L + (size_t)view * 12, *Km = K + (size_t)view * 12;
    float qa[3], qb[3];
    for (int i = 0; i < 3; ++i) qa[i] = affine_row(Lm + 4 * i, ax, ay, az), qb[i] = affine_row(Lm + 4 * i, bx, by, bz);
    const bool ina = qa[2] >= near, inb = qb[2] >= near;
    keep = keep && (ina || inb);
    if (ina != inb) {  // the end below the plane moves onto it, interpolated from the inner end
      const float *pi = ina ? qa : qb;
      float *po = ina ? qb : qa;
      const float tt = __fdiv_rn(__fsub_rn(pi[2], near), __fsub_rn(pi[2], po[2]));
      po[0] = __fadd_rn(pi[0], __fmul_rn(tt, __fsub_rn(po[0], pi[0])));
      po[1] = __fadd_rn(pi[1], __fmul_rn(tt, __fsub_rn(po[1], pi[1])));
      po[2] = near;
    }
    const float ha0 = affine_row(Km, qa[0], qa[1], qa[2]), ha1 = affine_row(Km + 4, qa[0], qa[1], qa[2]);
    const float ha2 = affine_row(Km + 8, qa[0], qa[1], qa[2]);
    const float hb0 = affine_row(Km, qb[0], qb[1], qb[2]), hb1 = affine_row(Km + 4, qb[0], qb[1], qb[2]);
    const float hb2 = affine_row(Km + 8, qb[0], qb[1], qb[2]);
    keep = keep && ha2 > 0.f && hb2 > 0.f;
    u0 = __fdiv_rn(ha0, ha2), v0 = __fdiv_rn(ha1, ha2), u1 = __fdiv_rn(hb0, hb2), v1 = __fdiv_rn(hb1, hb2);
  }
  const Seg s = make_record(keep, u0, v0, u1, v1, box, t, H, W);
  rec[idx] = s;
  boxes_px[idx] = make_int2(s.lo, s.hi);  // what the composite's cull reads: 8 bytes a record instead of 32
}

// is pixel centre (px, py), 1/32 pixel, within the capsule of s?  Selects only.  Bounds: visualize.py's module docstring.
__device__ __forceinline__ bool covers(const Seg &s, long long px, long long py) {
  const long long ex = px - 2ll * s.x0, ey = py - 2ll * s.y0;
  const long long dx = 2ll * (s.x1 - s.x0), dy = 2ll * (s.y1 - s.y0);
  const long long r2 = (long long)s.t * s.t, len2 = dx * dx + dy * dy, dot = dx * ex + dy * ey;
  const long long fx = ex - dx, fy = ey - dy;
  long long ca = dx * ey - dy * ex;
  ca = ca < 0 ? -ca : ca;
  const bool small = ca < kCrossLimit;
  const long long cs = small ? ca : 0;
  const bool first = dot <= 0, past = dot >= len2;
  const long long d2 = first ? ex * ex + ey * ey : fx * fx + fy * fy;
  return (first || past) ? d2 <= r2 : (small && cs * cs <= r2 * len2);
}

template <int S>
__global__ __launch_bounds__(kBlock) void vis_composite_kernel(const uint8_t *__restrict__ src, int H, int W,
                                                               const Seg *__restrict__ rec,
                                                               const int2 *__restrict__ boxes_px, int segs,
                                                               const int *__restrict__ colors, const int *__restrict__ cell_view,
                                                               int views, int cols, int h, int w,
                                                               uint8_t *__restrict__ out) {
  __shared__ __align__(16) Seg surv[kWaves][kWave];
  __shared__ int cnt[kWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const int cell = blockIdx.z, view = cell_view[cell];
  const int ox = blockIdx.x * kTileW + (t & (kTileW - 1)), oy = blockIdx.y * kTileH + t / kTileW;
  const bool live = ox < w && oy < h;
  uint8_t *dst = out + ((size_t)((cell / cols) * h + oy) * ((size_t)cols * w) + (size_t)(cell % cols) * w + ox) * 3;
  if (view < 0 || view >= views) {  // block-uniform: an unused cell is black; no view outside the block is ever read
    if (live) dst[0] = 0, dst[1] = 0, dst[2] = 0;
    return;
  }
  // the tile's source rectangle, inclusive (it may reach past the frame: record boxes are cut at the frame)
  const int tx0 = blockIdx.x * kTileW * S, tx1 = tx0 + kTileW * S - 1, ty0 = blockIdx.y * kTileH * S, ty1 = ty0 + kTileH * S - 1;
  const Seg *vrec = rec + (size_t)view * segs;
  const int2 *vbox = boxes_px + (size_t)view * segs;
  int best[S * S];
#pragma unroll
  for (int i = 0; i < S * S; ++i) best[i] = -1;
  for (int base = 0; base < segs; base += kChunk) {
    const int g = base + t;
    int2 bb = make_int2(kEmptyLo, 0);
    if (g < segs) bb = vbox[g];
    const int c0 = bb.x & 0xffff, r0 = bb.x >> 16, c1 = bb.y & 0xffff, r1 = bb.y >> 16;
    const bool hit = c0 <= c1 && r0 <= r1 && c0 <= tx1 && c1 >= tx0 && r0 <= ty1 && r1 >= ty0;
    const unsigned long long bal = __ballot(hit);
    if (hit) surv[wv][__popcll(bal & ((1ull << lane) - 1ull))] = vrec[g];  // hit implies g < segs
    if (lane == 0) cnt[wv] = __popcll(bal);
    __syncthreads();
    for (int k = 0; k < kWaves; ++k) {
      const int m = cnt[k];  // block-uniform
      for (int j = 0; j < m; ++j) {
        const Seg q = surv[k][j];  // every lane reads the same record: an LDS broadcast
#pragma unroll
        for (int sy = 0; sy < S; ++sy)
#pragma unroll
          for (int sx = 0; sx < S; ++sx) {
            const bool cov = covers(q, 32ll * (ox * S + sx) + 16, 32ll * (oy * S + sy) + 16);
            const int i = sy * S + sx;
            best[i] = (cov && q.box > best[i]) ? q.box : best[i];
          }
      }
    }
    __syncthreads();  // the lists are rewritten by the next chunk
  }
  if (!live) return;
  int sum0 = 0, sum1 = 0, sum2 = 0;
  const uint8_t *img = src + (size_t)view * H * W * 3;
#pragma unroll
  for (int sy = 0; sy < S; ++sy)
#pragma unroll
    for (int sx = 0; sx < S; ++sx) {
      const int b = best[sy * S + sx];
      if (b >= 0) {
        const int c = colors[b];
        sum0 += c & 255, sum1 += (c >> 8) & 255, sum2 += (c >> 16) & 255;
      } else {  // live: (oy S + sy, ox S + sx) < (h S, w S) <= (H, W)
        const uint8_t *p = img + ((size_t)(oy * S + sy) * W + (ox * S + sx)) * 3;
        sum0 += p[0], sum1 += p[1], sum2 += p[2];
      }
    }
  constexpr int kArea = S * S;
  dst[0] = (uint8_t)((sum0 + kArea / 2) / kArea);
  dst[1] = (uint8_t)((sum1 + kArea / 2) / kArea);
  dst[2] = (uint8_t)((sum2 + kArea / 2) / kArea);
}

// col = floor((x - ox) ppm), row = H - 1 - floor((y - oy) ppm) (oy the LOWER y limit); kept when both floors, compared as floats,
// lie in the canvas; the square spans [col - (p - 1) / 2, col + p / 2], cut at the canvas
__global__ __launch_bounds__(kBlock) void vis_points_kernel(const float *__restrict__ points, long long n, int C, float ox, float oy,
                                                            float ppm, int p, uint8_t *__restrict__ canvas, int H, int W) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float fc = floorf(__fmul_rn(__fsub_rn(points[(size_t)i * C], ox), ppm));
  const float fr = floorf(__fmul_rn(__fsub_rn(points[(size_t)i * C + 1], oy), ppm));
  if (!(fc >= 0.f && fc < (float)W && fr >= 0.f && fr < (float)H)) return;  // a NaN fails
  const int col = (int)fc, row = H - 1 - (int)fr;
  for (int rr = row - (p - 1) / 2; rr <= row + p / 2; ++rr) {
    if (rr < 0 || rr >= H) continue;
    for (int cc = col - (p - 1) / 2; cc <= col + p / 2; ++cc) {
      if (cc < 0 || cc >= W) continue;
      uint8_t *d = canvas + ((size_t)rr * W + cc) * 3;
      d[0] = 255, d[1] = 255, d[2] = 255;
    }
  }
}

// the records, then their pixel boxes again as a dense int2 array
size_t seg_bytes(long long views, long long n, long long edges) { return align_up((size_t)(views * n * edges) * sizeof(Seg), 256); }
size_t records_bytes(long long views, long long n, long long edges) {
  return seg_bytes(views, n, edges) + align_up((size_t)(views * n * edges) * sizeof(int2), 256);
}

bool shape_ok(int H, int W, int t) { return H >= 1 && H <= kMaxDim && W >= 1 && W <= kMaxDim && t >= 1 && t <= kMaxT; }

int launch_setup(const float *table, int n, const float *L, const float *K, int views, int bev, float near, float ox, float oy,
                 float ppm, int t, int H, int W, void *workspace, hipStream_t stream) {
  const long long total = (long long)views * n * (bev ? 4 : 12);
  if (total == 0) return BFHIP_OK;
  hipLaunchKernelGGL(vis_setup_kernel, dim3((unsigned)ceil_div(total, kBlock)), dim3(kBlock), 0, stream, table, n, L, K, views, bev,
                     near, ox, oy, ppm, t, H, W, (Seg *)workspace, (int2 *)((char *)workspace + seg_bytes(views, n, bev ? 4 : 12)));
  return check_launch("vis segment set-up");
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_vis_max_dim(void) { return kMaxDim; }
BFHIP_EXPORT int bfhip_vis_max_thickness(void) { return kMaxT; }
BFHIP_EXPORT int bfhip_vis_max_scale(void) { return kMaxScale; }

BFHIP_EXPORT size_t bfhip_vis_workspace_bytes(int n_views, int n_boxes, int edges) {
  if (n_views < 0 || n_boxes < 0 || (edges != 4 && edges != 12) || (long long)n_views * n_boxes * edges > 0x7fffffffll / 2) return 0;
  return records_bytes(n_views, n_boxes, edges);
}

BFHIP_EXPORT int bfhip_vis_camera_segments(const float *table, int n_boxes, const float *lidar2cam, const float *cam2img, int n_views,
                                           float near, int thickness, int H, int W, void *workspace, size_t workspace_bytes,
                                           void *stream) {
  BFHIP_REQUIRE(n_boxes >= 0 && n_views >= 1, "vis_camera_segments: %d boxes, %d views", n_boxes, n_views);
  BFHIP_REQUIRE((long long)n_views * n_boxes * 12 <= 0x7fffffffll / 2, "vis_camera_segments: %d views x %d boxes", n_views, n_boxes);
  BFHIP_REQUIRE(shape_ok(H, W, thickness), "vis_camera_segments: frame %d x %d (1 .. %d), thickness %d (1 .. %d)", H, W, kMaxDim,
                thickness, kMaxT);
  BFHIP_REQUIRE(near == near, "vis_camera_segments: near is NaN");
  BFHIP_REQUIRE(n_boxes == 0 || table, "vis_camera_segments: table is NULL with %d boxes", n_boxes);
  BFHIP_REQUIRE(lidar2cam && cam2img, "vis_camera_segments: lidar2cam or cam2img is NULL");
  BFHIP_REQUIRE((((uintptr_t)table | (uintptr_t)lidar2cam | (uintptr_t)cam2img) & 3) == 0, "vis_camera_segments: input not 4-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)workspace & 255) == 0, "vis_camera_segments: workspace not 256-byte aligned");
  const size_t need = records_bytes(n_views, n_boxes, 12);
  BFHIP_REQUIRE(workspace_bytes >= need && (workspace || need == 0), "vis_camera_segments: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  return launch_setup(table, n_boxes, lidar2cam, cam2img, n_views, 0, near, 0.f, 0.f, 0.f, thickness, H, W, workspace,
                      (hipStream_t)stream);
}

BFHIP_EXPORT int bfhip_vis_bev_segments(const float *table, int n_boxes, float x0, float y1, float px_per_m, int thickness, int H,
                                        int W, void *workspace, size_t workspace_bytes, void *stream) {
  BFHIP_REQUIRE(n_boxes >= 0 && (long long)n_boxes * 4 <= 0x7fffffffll / 2, "vis_bev_segments: %d boxes", n_boxes);
  BFHIP_REQUIRE(shape_ok(H, W, thickness), "vis_bev_segments: canvas %d x %d (1 .. %d), thickness %d (1 .. %d)", H, W, kMaxDim,
                thickness, kMaxT);
  BFHIP_REQUIRE(n_boxes == 0 || table, "vis_bev_segments: table is NULL with %d boxes", n_boxes);
  BFHIP_REQUIRE(((uintptr_t)table & 3) == 0, "vis_bev_segments: table not 4-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)workspace & 255) == 0, "vis_bev_segments: workspace not 256-byte aligned");
  const size_t need = records_bytes(1, n_boxes, 4);
  BFHIP_REQUIRE(workspace_bytes >= need && (workspace || need == 0), "vis_bev_segments: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  return launch_setup(table, n_boxes, nullptr, nullptr, 1, 1, 0.f, x0, y1, px_per_m, thickness, H, W, workspace, (hipStream_t)stream);
}

BFHIP_EXPORT int bfhip_vis_composite(const uint8_t *src, int n_views, int H, int W, const void *workspace, size_t workspace_bytes,
                                     int n_boxes, int edges, const int32_t *colors, const int32_t *cell_view, int rows, int cols,
                                     int scale, uint8_t *out, void *stream) {
  BFHIP_REQUIRE(n_views >= 1 && n_boxes >= 0 && (edges == 4 || edges == 12), "vis_composite: %d views, %d boxes, %d edges", n_views,
                n_boxes, edges);
  BFHIP_REQUIRE((long long)n_views * n_boxes * edges <= 0x7fffffffll / 2, "vis_composite: %d views x %d boxes", n_views, n_boxes);
  BFHIP_REQUIRE(shape_ok(H, W, 1), "vis_composite: frame %d x %d (1 .. %d a side)", H, W, kMaxDim);
  BFHIP_REQUIRE(scale >= 1 && scale <= kMaxScale && H / scale >= 1 && W / scale >= 1, "vis_composite: scale %d (1 .. %d) on %d x %d",
                scale, kMaxScale, H, W);
  BFHIP_REQUIRE(rows >= 1 && cols >= 1 && (long long)rows * cols <= 65535, "vis_composite: a grid of %d x %d cells", rows, cols);
  BFHIP_REQUIRE(src && out && cell_view && src != out, "vis_composite: src, out or cell_view is NULL, or src is out");
  BFHIP_REQUIRE(n_boxes == 0 || colors, "vis_composite: colors is NULL with %d boxes", n_boxes);
  BFHIP_REQUIRE((((uintptr_t)colors | (uintptr_t)cell_view) & 3) == 0, "vis_composite: colors or cell_view not 4-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)workspace & 255) == 0, "vis_composite: workspace not 256-byte aligned");
  const size_t need = records_bytes(n_views, n_boxes, edges);
  BFHIP_REQUIRE(workspace_bytes >= need && (workspace || need == 0), "vis_composite: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  const int h = H / scale, w = W / scale, segs = n_boxes * edges;
  const dim3 grid((unsigned)ceil_div(w, kTileW), (unsigned)ceil_div(h, kTileH), (unsigned)(rows * cols));
  const Seg *rec = (const Seg *)workspace;
  const int2 *boxes_px = (const int2 *)((const char *)workspace + seg_bytes(n_views, n_boxes, edges));
  hipStream_t s = (hipStream_t)stream;
#define BFHIP_VIS_LAUNCH(S) \
  hipLaunchKernelGGL(vis_composite_kernel<S>, grid, dim3(kBlock), 0, s, src, H, W, rec, boxes_px, segs, colors, cell_view, n_views, cols, h, w, out)
  switch (scale) {
    case 1: BFHIP_VIS_LAUNCH(1); break;
    case 2: BFHIP_VIS_LAUNCH(2); break;
    case 3: BFHIP_VIS_LAUNCH(3); break;
    default: BFHIP_VIS_LAUNCH(4); break;
  }
#undef BFHIP_VIS_LAUNCH
  return check_launch("vis composite");
}

BFHIP_EXPORT int bfhip_vis_bev_points(const float *points, long long n, int C, float x0, float y0, float px_per_m, int point_size,
                                      uint8_t *canvas, int H, int W, void *stream) {
  BFHIP_REQUIRE(n >= 0 && n < 0x80000000ll, "vis_bev_points: n=%lld (0 .. 2^31 - 1)", n);
  BFHIP_REQUIRE(C >= 2 && C <= 64, "vis_bev_points: %d columns (2 .. 64)", C);
  BFHIP_REQUIRE(point_size >= 1 && point_size <= 64, "vis_bev_points: point_size %d (1 .. 64)", point_size);
  BFHIP_REQUIRE(shape_ok(H, W, 1), "vis_bev_points: canvas %d x %d (1 .. %d a side)", H, W, kMaxDim);
  BFHIP_REQUIRE(canvas && (n == 0 || points), "vis_bev_points: canvas or points is NULL");
  BFHIP_REQUIRE(((uintptr_t)points & 3) == 0, "vis_bev_points: points not 4-byte aligned");
  if (n == 0) return BFHIP_OK;
  hipLaunchKernelGGL(vis_points_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, points, n, C, x0, y0,
                     px_per_m, point_size, canvas, H, W);
  return check_launch("vis bev points");
}
