// image_aug.hip -- ImageAug3D on the device (gfx950): PIL's resize (bicubic, antialiased, two passes with a uint8 image in
// between), crop (zero outside), mirror and nearest-neighbour rotation of raw uint8 camera frames [H, W, 3], followed by what
// preprocess.hip does (swap, normalise, pad, stack, cast, memory format).  Integers only up to the normalisation, so the pixels
// are PIL's bit for bit; the weights (22 fractional bits) and the rotation's 16.16 affine terms come from the host, which
// computes them in double as PIL does.
//
// Launch 1 (one per kMaxCams = 32 cameras), resize_crop_flip_kernel: one workgroup of 192 threads per 16 x 64 tile of a
// camera's cropped output.
//   * the tile's weights go to LDS once (row stride 27 ints: odd, so lanes on different columns hit different banks);
//   * horizontal pass: the source rows the tile's vertical taps need are staged kStageRows at a time -- aligned 4-byte
//     loads of the 3-byte-interleaved row segment, consecutive lanes consecutive dwords -- and thread (column, channel)
//     reduces its taps from the stage into hbuf[row][column * 3 + channel] as uint8 (PIL rounds between the passes);
//   * vertical pass: one wave per channel, lane = column, taps from hbuf; the store mirrors when the camera flips and
//     writes 0 where the crop lies outside the resized image.  Output: uint8 [cams, 3, fH, fW], every byte written once.
//   Only the source rows and columns the crop window needs are read.  LDS: 10 KiB stage + 23.25 KiB hbuf + 8.4 KiB weights.
// Launch 2: no camera of the batch rotates -> bfhip_img_preprocess on that intermediate.  Otherwise rotate_finish_kernel, the
//   same run-of-8 lanes, arithmetic and stores, with a per-pixel gather (x, y) = ((a2 + X a0 + Y a1) >> 16, (a5 + X a3 + Y a4)
//   >> 16), int32 with C's wrap, zero outside, for the cameras that rotate.
// GridMask (bfhip_image_aug_masked): when a sample of the batch carries an active mask record, launch 2 is
//   masked_finish_kernel, the finish kernel with the records of its cameras' samples as one more kernel argument.  The mask is
//   a closed form of the record -- bands of `length` every d on an hh x ww canvas, read at the pixel's canvas point or, when the
//   canvas rotates, through PIL's 16.16 affine with 0 outside -- so each lane computes the 8 bits of its run in registers (the
//   row test once per lane when the canvas does not rotate) and zeroes the masked pixels between the load and the
//   normalisation.  No mask image, no further launch or upload; without an active record the launches are as above.
//
// Bounds: at most kMaxTaps = 24 taps per output and in / out <= 6.25 per axis (resize >= 0.2 of any source of 39 pixels or more
// a side); bfhip_image_aug_supported() says so and the caller serves the rest in torch.  The per-camera descriptors travel in the
// kernel arguments, kMaxCams per launch (a larger batch is cut into chunks); the weight tables are the one device buffer the
// caller uploads.  The host validates every table entry against the source size before anything is launched.
#include <vector>

#include "common.h"
#include "img_store.h"

namespace bfhip {
namespace {

constexpr int kBlock = 192;      // kTW * 3: one thread per (column, channel) of the tile
constexpr int kTW = 64;          // tile of the cropped output
constexpr int kTH = 16;
constexpr int kMaxTaps = 24;
constexpr int kCoefStride = 27;  // lo, n, kMaxTaps weights, +1: odd
constexpr int kMaxSpanX = 424;   // source columns under one tile: (kTW + 3) * 6.25 + 1
constexpr int kMaxSpanY = 124;   // source rows under one tile:    (kTH + 3) * 6.25 + 1
constexpr int kStageRows = 8;
constexpr int kStageDwords = (kMaxSpanX * 3 + 3) / 4 + 2;
constexpr int kMaxCams = 32;     // descriptors per launch
constexpr int kFinishBlock = 256;

struct ResizeCam {
  const uint8_t *src;
  int h, w, crop_x, crop_y, flip;
  int h_off, h_taps, h_first, h_count;
  int v_off, v_taps, v_first, v_count;
  int pad_;
};
struct ResizeArgs {
  ResizeCam c[kMaxCams];
  int fH, fW;
};

__device__ __forceinline__ int clip8(int acc) {
  acc >>= 22;
  return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

__global__ __launch_bounds__(kBlock) void resize_crop_flip_kernel(ResizeArgs a, const int *__restrict__ tab,
                                                                   uint8_t *__restrict__ mid) {
  __shared__ unsigned stage[kStageRows * kStageDwords];
  __shared__ uint8_t hbuf[kMaxSpanY * kTW * 3];
  __shared__ int hcoef[kTW * kCoefStride];
  __shared__ int vcoef[kTH * kCoefStride];
  const ResizeCam &cam = a.c[blockIdx.z];
  const int t = threadIdx.x;
  const int x_t0 = blockIdx.x * kTW, y_t0 = blockIdx.y * kTH;  // the tile's origin in the crop
  // table entries [ia, ib) x [ja, jb) fall into this tile; entry i sits at local column i + xoff
  const int xoff = cam.h_first - cam.crop_x - x_t0, yoff = cam.v_first - cam.crop_y - y_t0;
  const int ia = max(0, -xoff), ib = min(cam.h_count, kTW - xoff);
  const int ja = max(0, -yoff), jb = min(cam.v_count, kTH - yoff);
  const bool any = ia < ib && ja < jb;  // block-uniform
  int sy0 = 0;

  if (any) {
    const int hs = 2 + cam.h_taps, vs = 2 + cam.v_taps;
    for (int e = t; e < (ib - ia) * hs; e += kBlock) {
      const int i = e / hs, f = e - i * hs;
      hcoef[(ia + i + xoff) * kCoefStride + f] = tab[cam.h_off + (ia + i) * hs + f];
    }
    for (int e = t; e < (jb - ja) * vs; e += kBlock) {
      const int j = e / vs, f = e - j * vs;
      vcoef[(ja + j + yoff) * kCoefStride + f] = tab[cam.v_off + (ja + j) * vs + f];
    }
    __syncthreads();
    const int *hlast = hcoef + (ib - 1 + xoff) * kCoefStride, *vlast = vcoef + (jb - 1 + yoff) * kCoefStride;
    const int sx0 = hcoef[(ia + xoff) * kCoefStride];
    sy0 = vcoef[(ja + yoff) * kCoefStride];
    const int nbytes = min(hlast[0] + hlast[1] - sx0, kMaxSpanX) * 3;
    const int nrows = min(vlast[0] + vlast[1] - sy0, kMaxSpanY);
    const uint8_t *frame = cam.src, *frame_end = cam.src + (size_t)cam.h * cam.w * 3;

    const int col = t / 3, c = t - col * 3;  // horizontal pass: channel fastest, as the source bytes lie
    const int i_mine = col - xoff;
    const bool hvalid = i_mine >= ia && i_mine < ib;
    const int *hc = hcoef + col * kCoefStride;
    const int hlo = hvalid ? hc[0] - sx0 : 0, hn = hvalid ? hc[1] : 0;

    for (int g = 0; g < nrows; g += kStageRows) {
      const int rows = min(kStageRows, nrows - g);
      for (int rr = 0; rr < rows; ++rr) {
        const uint8_t *p = frame + ((size_t)(sy0 + g + rr) * cam.w + sx0) * 3;
        const int shift = (int)((uintptr_t)p & 3);
        const int nd = (shift + nbytes + 3) >> 2;
        const uint8_t *p4 = p - shift;
        for (int d = t; d < nd; d += kBlock) {
          const uint8_t *q = p4 + 4 * d;
          unsigned v = 0;
          if (q >= frame && q + 4 <= frame_end) {
            v = *(const unsigned *)q;
          } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if (q + b >= frame && q + b < frame_end) v |= (unsigned)q[b] << (8 * b);
          }
          stage[rr * kStageDwords + d] = v;
        }
      }
      __syncthreads();
      if (hvalid) {
        for (int rr = 0; rr < rows; ++rr) {
          const int shift = (int)((uintptr_t)(frame + ((size_t)(sy0 + g + rr) * cam.w + sx0) * 3) & 3);
          const uint8_t *sb = (const uint8_t *)(stage + rr * kStageDwords) + shift + hlo * 3 + c;
          int acc = 1 << 21;
          for (int j = 0; j < hn; ++j) acc += (int)sb[j * 3] * hc[2 + j];
          hbuf[(g + rr) * (kTW * 3) + t] = (uint8_t)clip8(acc);
        }
      }
      __syncthreads();
    }
  }

  // vertical pass and store: one wave per channel, lane = column
  const int c2 = t / kTW, x = t - c2 * kTW;
  const int X = x_t0 + x;
  if (X >= a.fW) return;
  const int i_mine = x - xoff;
  const bool col_valid = any && i_mine >= ia && i_mine < ib;
  const int xs = cam.flip ? a.fW - 1 - X : X;
  uint8_t *plane = mid + ((size_t)blockIdx.z * 3 + c2) * a.fH * a.fW;
  for (int y = 0; y < kTH; ++y) {
    const int Y = y_t0 + y;
    if (Y >= a.fH) break;
    int val = 0;
    const int j_mine = y - yoff;
    if (col_valid && j_mine >= ja && j_mine < jb) {
      const int *vc = vcoef + y * kCoefStride;
      const uint8_t *hb = hbuf + (vc[0] - sy0) * (kTW * 3) + x * 3 + c2;
      const int n = vc[1];
      int acc = 1 << 21;
      for (int j = 0; j < n; ++j) acc += (int)hb[j * (kTW * 3)] * vc[2 + j];
      val = clip8(acc);
    }
    plane[(size_t)Y * a.fW + xs] = (uint8_t)val;
  }
}

struct FinishCam {
  int rotates;
  int a[6];
};
struct FinishArgs {
  FinishCam c[kMaxCams];
  float mean[3], std[3];
  float pad;
  int fH, fW, Hp, Wp, runs;
  int swap, normalise, out_vec;
};

// GridMask of one camera's sample (bfhip_grid_mask with the band counts folded in: bands_h = hh / d with use_h, otherwise 0)
struct MaskCam {
  int active, d, length, st_h, st_w, bands_h, bands_w, mode;
  int hh, ww, oy, ox, rotates;
  int a[6];
};
struct MaskArgs {
  MaskCam c[kMaxCams];
};

// canvas coordinate v lies in one of the `bands` bands of `length` every d from `start` on
__device__ __forceinline__ bool in_band(int v, int start, int d, int bands, int length) {
  const int t = v - start;
  if (t < 0) return false;
  const unsigned q = (unsigned)t / (unsigned)d;
  return q < (unsigned)bands && (unsigned)t - q * (unsigned)d < (unsigned)length;
}

// the mask's value (pixel stays) at canvas point (Y, X) of the unrotated canvas, or of the rotated one through the affine
__device__ __forceinline__ bool mask_keeps(const MaskCam &m, int Y, int X, bool row_band) {
  bool keep;
  if (m.rotates) {
    const int sx = (int)((unsigned)m.a[2] + (unsigned)X * (unsigned)m.a[0] + (unsigned)Y * (unsigned)m.a[1]) >> 16;
    const int sy = (int)((unsigned)m.a[5] + (unsigned)X * (unsigned)m.a[3] + (unsigned)Y * (unsigned)m.a[4]) >> 16;
    keep = sx >= 0 && sx < m.ww && sy >= 0 && sy < m.hh && !in_band(sy, m.st_h, m.d, m.bands_h, m.length) &&
           !in_band(sx, m.st_w, m.d, m.bands_w, m.length);
  } else {
    keep = !row_band && !in_band(X, m.st_w, m.d, m.bands_w, m.length);
  }
  return m.mode ? !keep : keep;
}

// O: output element (float / bf16_t); PIX: pixel-major [img, Hp, Wp, 3] output; MASK: mk holds the cameras' grid masks
template <typename O, bool PIX, bool MASK>
__device__ __forceinline__ void finish_run(const FinishArgs &a, const MaskArgs *mk, const uint8_t *__restrict__ mid,
                                           O *__restrict__ out) {
  const int img = blockIdx.y;
  const unsigned item = blockIdx.x * kFinishBlock + threadIdx.x;
  const int y = (int)(item / (unsigned)a.runs);
  if (y >= a.Hp) return;
  const int x0 = (int)(item - (unsigned)y * (unsigned)a.runs) * kRun;
  const int h = a.fH, w = a.fW;
  int nvalid = 0;
  if (y < h && x0 < w) nvalid = w - x0 < kRun ? w - x0 : kRun;
  const int nstore = a.Wp - x0 < kRun ? a.Wp - x0 : kRun;
  const bool vec = a.out_vec != 0;
  const FinishCam &cam = a.c[img];
  const bool rotates = cam.rotates != 0;

  int off[kRun];  // source offset in the plane, -1: outside the image
  if (rotates && nvalid > 0) {
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      const unsigned X = (unsigned)(x0 + j), Y = (unsigned)y;
      const int sx = (int)((unsigned)cam.a[2] + X * (unsigned)cam.a[0] + Y * (unsigned)cam.a[1]) >> 16;
      const int sy = (int)((unsigned)cam.a[5] + X * (unsigned)cam.a[3] + Y * (unsigned)cam.a[4]) >> 16;
      off[j] = (j < nvalid && sx >= 0 && sx < w && sy >= 0 && sy < h) ? sy * w + sx : -1;
    }
  }

  unsigned keep = 0xffu;  // bit j: pixel j of the run keeps its value under the sample's grid mask
  if (MASK && nvalid > 0 && mk->c[img].active) {
    const MaskCam &m = mk->c[img];
    const int Y = y + m.oy;
    const bool row_band = !m.rotates && in_band(Y, m.st_h, m.d, m.bands_h, m.length);  // one test per thread
    keep = 0;
#pragma unroll
    for (int j = 0; j < kRun; ++j) keep |= (mask_keeps(m, Y, x0 + j + m.ox, row_band) ? 1u : 0u) << j;
  }

  float val[3][kRun];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (nvalid > 0) {
      const int cs = a.swap ? 2 - c : c;
      const uint8_t *plane = mid + ((size_t)img * 3 + cs) * h * w;
      if (rotates) {
#pragma unroll
        for (int j = 0; j < kRun; ++j) val[c][j] = off[j] >= 0 ? (float)plane[off[j]] : 0.f;
      } else {
        load_run(plane + (size_t)y * w + x0, nvalid, val[c]);
      }
    }
    const float m = a.mean[c], sd = a.std[c];
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      float r = a.pad;
      if (j < nvalid) {
        const float v = MASK && !((keep >> j) & 1u) ? 0.f : val[c][j];
        r = a.normalise ? (v - m) / sd : v;
      }
      val[c][j] = r;
    }
  }

  if (PIX) {
    float e[3 * kRun];
#pragma unroll
    for (int j = 0; j < kRun; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) e[3 * j + c] = val[c][j];
    store_run<3 * kRun>(out + (((size_t)img * a.Hp + y) * a.Wp + x0) * 3, e, vec, 3 * nstore);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      store_run<kRun>(out + (((size_t)img * 3 + c) * a.Hp + y) * a.Wp + x0, val[c], vec, nstore);
  }
}

template <typename O, bool PIX>
__global__ __launch_bounds__(kFinishBlock) void rotate_finish_kernel(FinishArgs a, const uint8_t *__restrict__ mid,
                                                                     O *__restrict__ out) {
  finish_run<O, PIX, false>(a, nullptr, mid, out);
}

// the same with the samples' grid masks: a masked pixel is 0 in all three channels before the normalisation
template <typename O, bool PIX>
__global__ __launch_bounds__(kFinishBlock) void masked_finish_kernel(FinishArgs a, MaskArgs mk, const uint8_t *__restrict__ mid,
                                                                     O *__restrict__ out) {
  finish_run<O, PIX, true>(a, &mk, mid, out);
}

// mk: NULL, or the grid masks of the launch's cameras
template <typename O>
void launch_finish(const FinishArgs &a, const MaskArgs *mk, int images, int pixel_major, const uint8_t *mid, void *out,
                   hipStream_t s) {
  const dim3 grid(ceil_div((long long)a.Hp * a.runs, kFinishBlock), images);
  if (mk && pixel_major)
    hipLaunchKernelGGL((masked_finish_kernel<O, true>), grid, dim3(kFinishBlock), 0, s, a, *mk, mid, (O *)out);
  else if (mk)
    hipLaunchKernelGGL((masked_finish_kernel<O, false>), grid, dim3(kFinishBlock), 0, s, a, *mk, mid, (O *)out);
  else if (pixel_major)
    hipLaunchKernelGGL((rotate_finish_kernel<O, true>), grid, dim3(kFinishBlock), 0, s, a, mid, (O *)out);
  else
    hipLaunchKernelGGL((rotate_finish_kernel<O, false>), grid, dim3(kFinishBlock), 0, s, a, mid, (O *)out);
}

bool axis_supported(int in_size, int out_size, int taps) {
  return in_size >= 1 && out_size >= 1 && taps >= 0 && taps <= kMaxTaps && 4ll * in_size <= 25ll * out_size;
}

// One axis of one camera: the table block lies inside the tables, every entry reads inside the source, lo and lo + n do not
// decrease and no tile (any `tile` consecutive entries) spans more than `max_span` source elements.
int check_axis(const char *axis, int cam, const int32_t *tables, long long table_ints, int off, int taps, int first, int count,
               int crop, int size, int in_size, int tile, int max_span) {
  BFHIP_REQUIRE(count >= 0 && count <= size, "image_aug: camera %d %s: count %d of %d", cam, axis, count, size);
  if (count == 0) return BFHIP_OK;
  BFHIP_REQUIRE(taps >= 1 && taps <= kMaxTaps, "image_aug: camera %d %s: %d taps (1 .. %d)", cam, axis, taps, kMaxTaps);
  BFHIP_REQUIRE(first >= 0 && first >= crop && (long long)first + count <= (long long)crop + size,
                "image_aug: camera %d %s: window [%d, +%d) outside the crop [%d, +%d)", cam, axis, first, count, crop, size);
  const long long stride = 2 + taps;
  BFHIP_REQUIRE(off >= 0 && off + stride * count <= table_ints, "image_aug: camera %d %s: table [%d, +%lld) of %lld ints", cam,
                axis, off, stride * count, table_ints);
  const int32_t *e = tables + off;
  for (int i = 0; i < count; ++i) {
    const int lo = e[i * stride], n = e[i * stride + 1];
    BFHIP_REQUIRE(lo >= 0 && n >= 1 && n <= taps && (long long)lo + n <= in_size,
                  "image_aug: camera %d %s entry %d: lo=%d n=%d, source %d", cam, axis, i, lo, n, in_size);
    if (i > 0) {
      const int plo = e[(i - 1) * stride], pn = e[(i - 1) * stride + 1];
      BFHIP_REQUIRE(lo >= plo && lo + n >= plo + pn, "image_aug: camera %d %s entry %d: bounds decrease", cam, axis, i);
    }
    const int first_of_tile = i - tile + 1 > 0 ? i - tile + 1 : 0;
    BFHIP_REQUIRE(lo + n - e[first_of_tile * stride] <= max_span, "image_aug: camera %d %s entry %d: a tile spans %d source "
                  "elements (at most %d)", cam, axis, i, lo + n - e[first_of_tile * stride], max_span);
  }
  return BFHIP_OK;
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_image_aug_max_taps(void) { return kMaxTaps; }
BFHIP_EXPORT int bfhip_image_aug_max_cams(void) { return kMaxCams; }

BFHIP_EXPORT int bfhip_image_aug_supported(int src_h, int src_w, int new_h, int new_w, int fH, int fW, int h_taps, int v_taps) {
  return (fH >= 1 && fW >= 1 && (long long)src_h * src_w * 3 <= 0x7fffffffll && (long long)fH * fW <= 0x7fffffffll / 3 &&
          axis_supported(src_w, new_w, h_taps) && axis_supported(src_h, new_h, v_taps))
             ? 1
             : 0;
}

BFHIP_EXPORT int bfhip_image_aug(const bfhip_image_aug_cam *cams_host, int n_samples, int views, const int32_t *tables_host,
                                 const int32_t *tables_dev, long long table_ints, int fH, int fW, void *mid, int swap_rb,
                                 int normalise, const float *mean_host, const float *std_host, float pad_value, int Hp, int Wp,
                                 int out_dtype, int pixel_major, void *out, void *stream) {
  return bfhip_image_aug_masked(cams_host, nullptr, n_samples, views, tables_host, tables_dev, table_ints, fH, fW, mid, swap_rb,
                                normalise, mean_host, std_host, pad_value, Hp, Wp, out_dtype, pixel_major, out, stream);
}

BFHIP_EXPORT int bfhip_image_aug_masked(const bfhip_image_aug_cam *cams_host, const bfhip_grid_mask *masks_host, int n_samples,
                                        int views, const int32_t *tables_host, const int32_t *tables_dev, long long table_ints,
                                        int fH, int fW, void *mid, int swap_rb, int normalise, const float *mean_host,
                                        const float *std_host, float pad_value, int Hp, int Wp, int out_dtype, int pixel_major,
                                        void *out, void *stream) {
  BFHIP_REQUIRE(cams_host && tables_host && tables_dev && mid && out, "image_aug: a required pointer is NULL");
  BFHIP_REQUIRE(n_samples >= 1 && views >= 1 && (long long)n_samples * views <= 0x7fffffffll / 3,
                "image_aug: n_samples=%d views=%d", n_samples, views);
  BFHIP_REQUIRE(fH >= 1 && fW >= 1 && (long long)fH * fW <= 0x7fffffffll / 3, "image_aug: final size %d x %d", fH, fW);
  BFHIP_REQUIRE(Hp >= fH && Wp >= fW && (long long)Hp * ((Wp + kRun - 1) / kRun) <= 0x7fffffffll,
                "image_aug: padded size %d x %d below the final %d x %d", Hp, Wp, fH, fW);
  BFHIP_REQUIRE(out_dtype == 0 || out_dtype == 1, "image_aug: out_dtype %d (0 = float32, 1 = bf16)", out_dtype);
  BFHIP_REQUIRE(!normalise || (mean_host && std_host), "image_aug: normalise needs mean_host and std_host");
  BFHIP_REQUIRE(table_ints >= 1 && table_ints <= 0x7fffffffll, "image_aug: table_ints=%lld", table_ints);
  const int cams = n_samples * views;
  bool any_rotates = false;
  for (int i = 0; i < cams; ++i) {
    const bfhip_image_aug_cam &c = cams_host[i];
    BFHIP_REQUIRE(c.data && c.h >= 1 && c.w >= 1 && (long long)c.h * c.w * 3 <= 0x7fffffffll,
                  "image_aug: camera %d: data=%p h=%d w=%d", i, c.data, c.h, c.w);
    int rc = check_axis("x", i, tables_host, table_ints, c.h_off, c.h_taps, c.h_first, c.h_count, c.crop[0], fW, c.w, kTW,
                        kMaxSpanX);
    if (rc != BFHIP_OK) return rc;
    rc = check_axis("y", i, tables_host, table_ints, c.v_off, c.v_taps, c.v_first, c.v_count, c.crop[1], fH, c.h, kTH, kMaxSpanY);
    if (rc != BFHIP_OK) return rc;
    any_rotates = any_rotates || c.rotates != 0;
  }
  bool any_mask = false;
  for (int i = 0; masks_host && i < n_samples; ++i) {
    const bfhip_grid_mask &g = masks_host[i];
    if (!g.active) continue;
    BFHIP_REQUIRE(g.d >= 2 && g.length >= 1 && g.length < g.d && g.st_h >= 0 && g.st_h < g.d && g.st_w >= 0 && g.st_w < g.d,
                  "image_aug: sample %d grid mask: d=%d length=%d st_h=%d st_w=%d (d >= 2, 1 <= length < d, 0 <= st < d)", i, g.d,
                  g.length, g.st_h, g.st_w);
    BFHIP_REQUIRE(g.hh >= 1 && g.ww >= 1 && g.crop[0] >= 0 && g.crop[1] >= 0 && (long long)g.crop[0] + fH <= g.hh &&
                      (long long)g.crop[1] + fW <= g.ww,
                  "image_aug: sample %d grid mask: window [%d, +%d) x [%d, +%d) outside the canvas %d x %d", i, g.crop[0], fH,
                  g.crop[1], fW, g.hh, g.ww);
    any_mask = true;
  }

  const dim3 tiles(ceil_div(fW, kTW), ceil_div(fH, kTH));
  BFHIP_REQUIRE(tiles.y <= 65535u, "image_aug: final height %d", fH);
  ResizeArgs ra;
  ra.fH = fH;
  ra.fW = fW;
  for (int first = 0; first < cams; first += kMaxCams) {
    const int n = cams - first < kMaxCams ? cams - first : kMaxCams;
    for (int i = 0; i < kMaxCams; ++i) {
      const bfhip_image_aug_cam &c = cams_host[first + (i < n ? i : 0)];
      ResizeCam &r = ra.c[i];
      r.src = (const uint8_t *)c.data;
      r.h = c.h, r.w = c.w, r.crop_x = c.crop[0], r.crop_y = c.crop[1], r.flip = c.flip ? 1 : 0;
      r.h_off = c.h_off, r.h_taps = c.h_taps, r.h_first = c.h_first, r.h_count = c.h_count;
      r.v_off = c.v_off, r.v_taps = c.v_taps, r.v_first = c.v_first, r.v_count = c.v_count;
      r.pad_ = 0;
    }
    hipLaunchKernelGGL(resize_crop_flip_kernel, dim3(tiles.x, tiles.y, n), dim3(kBlock), 0, (hipStream_t)stream, ra, tables_dev,
                       (uint8_t *)mid + (size_t)first * 3 * fH * fW);
    const int rc = check_launch("image_aug resize");
    if (rc != BFHIP_OK) return rc;
  }

  if (!any_rotates && !any_mask) {  // the second launch is the preprocessing kernel itself on the uint8 intermediate
    std::vector<bfhip_img_desc> descs(n_samples);  // bfhip_img_preprocess cuts a long list into launches itself
    for (int i = 0; i < n_samples; ++i) {
      descs[i].data = (const uint8_t *)mid + (size_t)i * views * 3 * fH * fW;
      descs[i].h = fH;
      descs[i].w = fW;
    }
    return bfhip_img_preprocess(descs.data(), n_samples, views, 0, swap_rb, normalise, mean_host, std_host, pad_value, Hp, Wp,
                                out_dtype, pixel_major, out, stream);
  }

  FinishArgs fa;
  for (int c = 0; c < 3; ++c) {
    fa.mean[c] = normalise ? mean_host[c] : 0.f;
    fa.std[c] = normalise ? std_host[c] : 1.f;
  }
  fa.pad = pad_value;
  fa.fH = fH, fa.fW = fW, fa.Hp = Hp, fa.Wp = Wp;
  fa.runs = (Wp + kRun - 1) / kRun;
  fa.swap = swap_rb ? 1 : 0;
  fa.normalise = normalise ? 1 : 0;
  const size_t cam_bytes = (size_t)3 * Hp * Wp * (out_dtype == 1 ? 2 : 4);
  MaskArgs ma;
  for (int first = 0; first < cams; first += kMaxCams) {
    const int n = cams - first < kMaxCams ? cams - first : kMaxCams;
    for (int i = 0; i < kMaxCams; ++i) {
      const int cam = first + (i < n ? i : 0);
      const bfhip_image_aug_cam &c = cams_host[cam];
      fa.c[i].rotates = c.rotates ? 1 : 0;
      for (int k = 0; k < 6; ++k) fa.c[i].a[k] = c.a[k];
      if (!any_mask) continue;
      const bfhip_grid_mask &g = masks_host[cam / views];  // the mask is the sample's: a chunk may begin inside one
      MaskCam &m = ma.c[i];
      m.active = g.active ? 1 : 0;
      m.d = g.active ? g.d : 1, m.length = g.length, m.st_h = g.st_h, m.st_w = g.st_w;
      m.bands_h = g.active && g.use_h ? g.hh / g.d : 0, m.bands_w = g.active && g.use_w ? g.ww / g.d : 0;
      m.mode = g.mode ? 1 : 0;
      m.hh = g.hh, m.ww = g.ww, m.oy = g.crop[0], m.ox = g.crop[1], m.rotates = g.rotates ? 1 : 0;
      for (int k = 0; k < 6; ++k) m.a[k] = g.a[k];
    }
    char *dst = (char *)out + (size_t)first * cam_bytes;
    const uint8_t *src = (const uint8_t *)mid + (size_t)first * 3 * fH * fW;
    fa.out_vec = (Wp % kRun == 0 && ((uintptr_t)dst & 15) == 0) ? 1 : 0;
    const MaskArgs *mk = any_mask ? &ma : nullptr;
    if (out_dtype == 1) launch_finish<bf16_t>(fa, mk, n, pixel_major, src, dst, (hipStream_t)stream);
    else launch_finish<float>(fa, mk, n, pixel_major, src, dst, (hipStream_t)stream);
    const int rc = check_launch("image_aug finish");
    if (rc != BFHIP_OK) return rc;
  }
  return BFHIP_OK;
}
