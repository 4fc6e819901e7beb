// jpeg.hip -- JPEG decode split at the entropy stage.  The host half (csrc/jpeg_host.h: markers + Huffman, no HIP call) leaves
// int16 coefficient blocks; the device half here turns a whole batch of frames into interleaved RGB in two launches:
//   1. jpeg_idct_kernel   dequantise + libjpeg's accurate integer 8x8 inverse DCT -> uint8 component planes, whole blocks
//   2. jpeg_colour_kernel libjpeg's triangle-filter chroma upsampling + 16-bit fixed-point YCbCr -> RGB, [H, W, 3] uint8
// Both are defined on every input by bevfusion_amd/jpeg.py (torch_jpeg_decode): all sums and products are 32-bit
// two's-complement wrap-around, done on uint32_t and cast only for the arithmetic shifts.
#include "common.h"
#include "jpeg_host.h"

namespace bfhip {

typedef uint32_t U;

// One pass of the 8-point inverse DCT of libjpeg's jidctint ("islow", CONST_BITS = 13), descaled by `shift` with rounding.
template <int shift>
__device__ __forceinline__ void idct_1d(const int32_t *in, int32_t *out) {
  const U i0 = (U)in[0], i1 = (U)in[1], i2 = (U)in[2], i3 = (U)in[3], i4 = (U)in[4], i5 = (U)in[5], i6 = (U)in[6], i7 = (U)in[7];
  U z1 = (i2 + i6) * (U)4433;
  const U e2 = z1 + i6 * (U)(-15137);
  const U e3 = z1 + i2 * (U)6270;
  const U e0 = (i0 + i4) << 13, e1 = (i0 - i4) << 13;
  const U t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  U o0 = i7, o1 = i5, o2 = i3, o3 = i1;
  z1 = o0 + o3;
  U z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const U z5 = (z3 + z4) * (U)9633;
  o0 *= (U)2446; o1 *= (U)16819; o2 *= (U)25172; o3 *= (U)12299;
  z1 *= (U)(-7373); z2 *= (U)(-20995); z3 *= (U)(-16069); z4 *= (U)(-3196);
  z3 += z5; z4 += z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  const U half = (U)1 << (shift - 1);
  out[0] = (int32_t)(t10 + o3 + half) >> shift; out[7] = (int32_t)(t10 - o3 + half) >> shift;
  out[1] = (int32_t)(t11 + o2 + half) >> shift; out[6] = (int32_t)(t11 - o2 + half) >> shift;
  out[2] = (int32_t)(t12 + o1 + half) >> shift; out[5] = (int32_t)(t12 - o1 + half) >> shift;
  out[3] = (int32_t)(t13 + o0 + half) >> shift; out[4] = (int32_t)(t13 - o0 + half) >> shift;
}

constexpr int kIdctThreads = 256;               // 8 lanes a block
constexpr int kIdctBlocks = kIdctThreads / 8;   // 8x8 blocks a workgroup
constexpr int kTileStride = 9;                  // int32 row stride of a block's tile: rows and columns both conflict-free

// grid (ceil(most blocks of a frame / 32), n_frames).  Lane l of a block loads coefficient row l (one 16-byte load) and its
// quantisation row, leaves the products in the tile, runs column l, then row l, and stores the row's 8 pixels at once.
__global__ __launch_bounds__(kIdctThreads) void jpeg_idct_kernel(const bfhip_jpeg_frame *__restrict__ frames,
                                                                const int16_t *__restrict__ coef, uint8_t *__restrict__ planes) {
  __shared__ int32_t tile[kIdctBlocks][8 * kTileStride];
  const bfhip_jpeg_frame &f = frames[blockIdx.y];
  const long long n0 = (long long)f.block_cols[0] * f.block_rows[0], n1 = (long long)f.block_cols[1] * f.block_rows[1];
  const long long total = n0 + n1 + (long long)f.block_cols[2] * f.block_rows[2];
  if ((long long)blockIdx.x * kIdctBlocks >= total) return;  // the whole workgroup: this frame has fewer blocks
  const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
  long long b = (long long)blockIdx.x * kIdctBlocks + slot;
  const bool live = b < total;
  if (!live) b = 0;
  const int c = b < n0 ? 0 : (b < n0 + n1 ? 1 : 2);
  b -= c == 0 ? 0 : (c == 1 ? n0 : n0 + n1);
  int32_t *t = tile[slot];
  int32_t v[8], w[8];
  if (live) {
    const uint4 raw = *reinterpret_cast<const uint4 *>(coef + f.coef_off[c] + b * 64 + lane * 8);
    const uint4 q = *reinterpret_cast<const uint4 *>(&f.quant[c][lane * 8]);
    const U rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[lane * kTileStride + 2 * j] = (int32_t)(int16_t)(rw[j] & 0xffffu) * (int32_t)(qw[j] & 0xffffu);
      t[lane * kTileStride + 2 * j + 1] = (int32_t)(int16_t)(rw[j] >> 16) * (int32_t)(qw[j] >> 16);
    }
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = t[r * kTileStride + lane];
    idct_1d<11>(v, w);  // CONST_BITS - PASS1_BITS
#pragma unroll
    for (int r = 0; r < 8; ++r) t[r * kTileStride + lane] = w[r];
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int x = 0; x < 8; ++x) v[x] = t[lane * kTileStride + x];
    idct_1d<18>(v, w);  // CONST_BITS + PASS1_BITS + 3
    U lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (U)min(max(w[x] + 128, 0), 255) << (8 * x);
      hi |= (U)min(max(w[x + 4] + 128, 0), 255) << (8 * x);
    }
    const long long bc = f.block_cols[c], brow = b / bc, bcol = b - brow * bc;
    uint8_t *dst = planes + f.plane_off[c] + (brow * 8 + lane) * (bc * 8) + bcol * 8;
    *reinterpret_cast<uint2 *>(dst) = make_uint2(lo, hi);
  }
}

constexpr int kRun = 8;  // output pixels of one row a thread makes: 24 bytes, three 8-byte stores
constexpr int kColourThreads = 256;

struct ChromaPlane {
  const uint8_t *p;
  long long stride;
  int w, h;  // the component's real extent: neighbours are clamped to it
};

// The chroma sample libjpeg's upsampler gives output pixel (x, y).  Its triangle filters run when the component is more than
// two samples wide (h2v1, h2v2) and always for h1v2; narrower h2 components are replicated.
__device__ __forceinline__ int upsample(const ChromaPlane &c, int x, int y, int hs, int vs) {
  if (hs == 1 && vs == 1) return c.p[y * c.stride + x];
  if (hs == 2 && c.w <= 2) return c.p[(vs == 2 ? y >> 1 : y) * c.stride + (x >> 1)];
  if (vs == 1) {
    const int cx = x >> 1, odd = x & 1, nb = odd ? min(cx + 1, c.w - 1) : max(cx - 1, 0);
    return (3 * (int)c.p[y * c.stride + cx] + (int)c.p[y * c.stride + nb] + (odd ? 2 : 1)) >> 2;
  }
  const int cy = y >> 1, oddy = y & 1, fy = oddy ? min(cy + 1, c.h - 1) : max(cy - 1, 0);
  const uint8_t *near = c.p + cy * c.stride, *far = c.p + fy * c.stride;
  if (hs == 1) return (3 * (int)near[x] + (int)far[x] + (oddy ? 2 : 1)) >> 2;
  const int cx = x >> 1, odd = x & 1, nb = odd ? min(cx + 1, c.w - 1) : max(cx - 1, 0);
  const int here = 3 * (int)near[cx] + (int)far[cx], there = 3 * (int)near[nb] + (int)far[nb];
  return (3 * here + there + (odd ? 7 : 8)) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// The six h2v2 column sums 3 * near + far of chroma columns cx0 - 1 .. cx0 + 4 (the outer two clamped to the real extent): what
// the eight pixels over columns cx0 .. cx0 + 3 need.  One aligned 4-byte load and two byte loads a row.
__device__ __forceinline__ void column_sums(const ChromaPlane &c, int cx0, int cy, int fy, int *s) {
  const uint8_t *near = c.p + cy * c.stride, *far = c.p + fy * c.stride;
  const int lx = max(cx0 - 1, 0), rx = min(cx0 + 4, c.w - 1);
  const U nw = *reinterpret_cast<const U *>(near + cx0), fw = *reinterpret_cast<const U *>(far + cx0);
  s[0] = 3 * (int)near[lx] + (int)far[lx];
#pragma unroll
  for (int j = 0; j < 4; ++j) s[1 + j] = 3 * (int)((nw >> (8 * j)) & 0xffu) + (int)((fw >> (8 * j)) & 0xffu);
  s[5] = 3 * (int)near[rx] + (int)far[rx];
}

// grid (ceil(most runs of a frame / 256), n_frames); a thread makes pixels [x0, x0 + 8) of one row.  A whole run of a 4:2:0
// frame (the common case) reads its chroma as words; every other run goes through upsample() sample by sample -- the same
// values.  A workgroup whose 256 runs are whole and lie end to end in the output (W a multiple of 8) hands its 6144 bytes
// through LDS so that consecutive lanes store consecutive 8 bytes; otherwise every thread stores its own 24.
__global__ __launch_bounds__(kColourThreads) void jpeg_colour_kernel(const bfhip_jpeg_frame *__restrict__ frames,
                                                                    const uint8_t *__restrict__ planes, uint8_t *__restrict__ rgb) {
  __shared__ uint2 stage[3 * kColourThreads];
  const bfhip_jpeg_frame &f = frames[blockIdx.y];
  const int W = f.width, H = f.height, hs = f.hs, vs = f.vs;
  const long long runs_per_row = (W + kRun - 1) / kRun, runs = runs_per_row * H;
  const long long first = (long long)blockIdx.x * kColourThreads, run = first + threadIdx.x;
  uint8_t *block_dst = rgb + f.rgb_off + first * (3 * kRun);
  // uniform over the workgroup: all 256 runs exist, are whole, and follow one another in memory
  const bool dense = W % kRun == 0 && first + kColourThreads <= runs && (reinterpret_cast<uintptr_t>(block_dst) & 7) == 0;
  if (run >= runs) return;
  const int y = (int)(run / runs_per_row), x0 = (int)(run - (long long)y * runs_per_row) * kRun;
  const int n = min(kRun, W - x0);
  const uint8_t *luma = planes + f.plane_off[0] + (long long)y * (f.block_cols[0] * 8) + x0;
  ChromaPlane cb, cr;
  cb.p = planes + f.plane_off[1];
  cr.p = planes + f.plane_off[2];
  cb.stride = (long long)f.block_cols[1] * 8;
  cr.stride = (long long)f.block_cols[2] * 8;
  cb.w = cr.w = (W + hs - 1) / hs;
  cb.h = cr.h = (H + vs - 1) / vs;
  const uint2 yy = *reinterpret_cast<const uint2 *>(luma);  // x0 is a multiple of 8 and the plane's width one as well
  int ub[kRun], ur[kRun];
  if (hs == 2 && vs == 2 && cb.w > 2 && n == kRun) {
    const int cy = y >> 1, fy = (y & 1) ? min(cy + 1, cb.h - 1) : max(cy - 1, 0);
    int sb[6], sr[6];
    column_sums(cb, x0 >> 1, cy, fy, sb);
    column_sums(cr, x0 >> 1, cy, fy, sr);
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      const int j = 1 + (i >> 1), k = (i & 1) ? j + 1 : j - 1, bias = (i & 1) ? 7 : 8;
      ub[i] = (3 * sb[j] + sb[k] + bias) >> 4;
      ur[i] = (3 * sr[j] + sr[k] + bias) >> 4;
    }
  } else {
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      const int x = min(x0 + i, W - 1);  // the tail of a partial run repeats the last pixel and is not stored
      ub[i] = upsample(cb, x, y, hs, vs);
      ur[i] = upsample(cr, x, y, hs, vs);
    }
  }
  uint8_t px[3 * kRun];
#pragma unroll
  for (int i = 0; i < kRun; ++i) {
    const int yv = (int)(((i < 4 ? yy.x : yy.y) >> (8 * (i & 3))) & 0xffu);
    const U b = (U)(ub[i] - 128), r = (U)(ur[i] - 128);
    px[3 * i + 0] = (uint8_t)clamp255(yv + ((int32_t)((U)91881 * r + 32768u) >> 16));
    px[3 * i + 1] = (uint8_t)clamp255(yv + ((int32_t)((U)(-22554) * b + (U)(-46802) * r + 32768u) >> 16));
    px[3 * i + 2] = (uint8_t)clamp255(yv + ((int32_t)((U)116130 * b + 32768u) >> 16));
  }
  uint2 packed[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    U lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo |= (U)px[8 * k + j] << (8 * j);
      hi |= (U)px[8 * k + 4 + j] << (8 * j);
    }
    packed[k] = make_uint2(lo, hi);
  }
  if (dense) {
#pragma unroll
    for (int k = 0; k < 3; ++k) stage[3 * threadIdx.x + k] = packed[k];
    __syncthreads();
    uint2 *d2 = reinterpret_cast<uint2 *>(block_dst);
#pragma unroll
    for (int k = 0; k < 3; ++k) d2[k * kColourThreads + threadIdx.x] = stage[k * kColourThreads + threadIdx.x];
    return;
  }
  uint8_t *dst = rgb + f.rgb_off + ((long long)y * W + x0) * 3;
  if (n == kRun && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
    uint2 *d2 = reinterpret_cast<uint2 *>(dst);
#pragma unroll
    for (int k = 0; k < 3; ++k) d2[k] = packed[k];
  } else {
    for (int i = 0; i < 3 * n; ++i) dst[i] = px[i];
  }
}

}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_jpeg_parse(const uint8_t *bytes, size_t n, bfhip_jpeg_header *header) {
  BFHIP_REQUIRE(header != nullptr, "bfhip_jpeg_parse: null header");
  char err[bfjpeg::kErrLen];
  const int rc = bfjpeg::parse(bytes, n, header, nullptr, err);
  if (rc) set_error("%s", err);
  return rc;
}

BFHIP_EXPORT int bfhip_jpeg_entropy_decode(const uint8_t *bytes, size_t n, const bfhip_jpeg_header *header, int16_t *coef,
                                           size_t coef_bytes) {
  char err[bfjpeg::kErrLen];
  const int rc = bfjpeg::entropy_decode(bytes, n, header, coef, coef_bytes, err);
  if (rc) set_error("%s", err);
  return rc;
}

BFHIP_EXPORT int bfhip_jpeg_decode(const bfhip_jpeg_frame *frames_host, const bfhip_jpeg_frame *frames_dev, int n_frames,
                                   const int16_t *coef_dev, size_t coef_elems, uint8_t *planes_dev, size_t planes_bytes,
                                   uint8_t *rgb_dev, size_t rgb_bytes, void *stream) {
  BFHIP_REQUIRE(frames_host && frames_dev && coef_dev && planes_dev && rgb_dev, "bfhip_jpeg_decode: null argument");
  BFHIP_REQUIRE(n_frames >= 1 && n_frames <= 65535, "bfhip_jpeg_decode: n_frames=%d outside 1..65535", n_frames);
  BFHIP_REQUIRE((reinterpret_cast<uintptr_t>(coef_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(planes_dev) & 7) == 0 &&
                (reinterpret_cast<uintptr_t>(frames_dev) & 15) == 0,
                "bfhip_jpeg_decode: coef_dev / frames_dev must be 16-byte and planes_dev 8-byte aligned");
  long long most_blocks = 0, most_runs = 0;
  for (int i = 0; i < n_frames; ++i) {
    const bfhip_jpeg_frame &f = frames_host[i];
    BFHIP_REQUIRE(f.width >= 1 && f.height >= 1 && f.width <= 65535 && f.height <= 65535 && (f.hs == 1 || f.hs == 2) &&
                  (f.vs == 1 || f.vs == 2), "bfhip_jpeg_decode: frame %d: %dx%d sampling %dx%d", i, f.width, f.height, f.hs, f.vs);
    const int mx = (f.width + 8 * f.hs - 1) / (8 * f.hs), my = (f.height + 8 * f.vs - 1) / (8 * f.vs);
    long long blocks = 0;
    for (int c = 0; c < 3; ++c) {
      BFHIP_REQUIRE(f.block_cols[c] == mx * (c ? 1 : f.hs) && f.block_rows[c] == my * (c ? 1 : f.vs),
                    "bfhip_jpeg_decode: frame %d component %d: %d x %d blocks do not fit the frame", i, c, f.block_rows[c], f.block_cols[c]);
      const long long nb = (long long)f.block_cols[c] * f.block_rows[c];
      BFHIP_REQUIRE(f.coef_off[c] >= 0 && f.coef_off[c] % 8 == 0 && (unsigned long long)(f.coef_off[c] + nb * 64) <= coef_elems,
                    "bfhip_jpeg_decode: frame %d component %d: coefficients outside the buffer", i, c);
      BFHIP_REQUIRE(f.plane_off[c] >= 0 && f.plane_off[c] % 8 == 0 && (unsigned long long)(f.plane_off[c] + nb * 64) <= planes_bytes,
                    "bfhip_jpeg_decode: frame %d component %d: plane outside the buffer", i, c);
      blocks += nb;
    }
    BFHIP_REQUIRE(f.rgb_off >= 0 && (unsigned long long)(f.rgb_off + (long long)f.width * f.height * 3) <= rgb_bytes,
                  "bfhip_jpeg_decode: frame %d: pixels outside the output block", i);
    most_blocks = blocks > most_blocks ? blocks : most_blocks;
    const long long runs = (long long)((f.width + kRun - 1) / kRun) * f.height;
    most_runs = runs > most_runs ? runs : most_runs;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)ceil_div(most_blocks, kIdctBlocks), (unsigned)n_frames), dim3(kIdctThreads), 0, s,
                     frames_dev, coef_dev, planes_dev);
  int rc = check_launch("jpeg_idct_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)ceil_div(most_runs, kColourThreads), (unsigned)n_frames), dim3(kColourThreads),
                     0, s, frames_dev, planes_dev, rgb_dev);
  return check_launch("jpeg_colour_kernel");
}
