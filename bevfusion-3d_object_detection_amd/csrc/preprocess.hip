// preprocess.hip -- Det3DDataPreprocessor's image path in one pass (gfx950): channel swap, u8 / f32 -> fp32, (x - mean) / std,
// pad at the bottom and right, stack the ragged per-sample [views, 3, h, w] blocks into one batch, cast to the output dtype and
// write the memory format the backbone's first convolution reads.
//
//   out[b, v, c, y, x] = y < h_b && x < w_b ? (float(src_b[v, c', y, x]) - mean[c]) / std[c] : pad_value       c' = swap ? 2 - c : c
//
// fp32, subtraction first, a true division (the library's build flags keep both IEEE: no contraction, correctly rounded
// divide), so the result is bit for bit what torch computes; bf16 output rounds that value once, to nearest even.  A padded
// element is pad_value itself.  Every output element is written exactly once: the caller needs no memset.
//
// No reuse, so no LDS: a lane owns a run of kRun = 8 consecutive pixels of one output row of one view and handles the three
// channels of that run.  Reads are one 8-byte (u8) or two 16-byte (f32) loads per plane, stores are 16 bytes: per plane 16 B
// (bf16) or 2 x 16 B (f32) when planar; pixel-major, the lane's 24 values are one contiguous 48 B (bf16: 3 stores) or 96 B
// (f32: 6 stores) piece and consecutive lanes continue each other.  The vector load needs the whole run inside the image and
// an aligned address, the vector store needs Wp % 8 == 0 and a 16-byte aligned output; everything else -- a run across the
// image's right edge, a row width that is no multiple of 8, a source that starts at an odd byte -- goes element by element
// through the same arithmetic.  A run that lies wholly in the padding loads nothing.
//
// blockIdx.y is the (sample, view) image, so the sample's descriptor (passed by value in the kernel arguments: no device
// table, no copy) is read with a block-uniform index; blockIdx.x walks the image's Hp * ceil(Wp / 8) runs.
#include "common.h"
#include "img_store.h"

namespace bfhip {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxSamples = 32;  // descriptors per launch (512 bytes of kernel arguments)
constexpr int kMaxViews = 1024;  // kMaxSamples * views images = gridDim.y

struct Args {
  bfhip_img_desc s[kMaxSamples];
  float mean[3], std[3];
  float pad;
  int views, Hp, Wp, runs;  // runs = ceil(Wp / kRun)
  int swap, normalise;
  int out_vec;              // Wp % kRun == 0 and a 16-byte aligned output: every store is a 16-byte vector
};

// S: source element (uint8_t / float); O: output element (float / bf16_t); PIX: pixel-major [img, Hp, Wp, 3] output
template <typename S, typename O, bool PIX>
__global__ __launch_bounds__(kBlock) void img_preprocess_kernel(Args a, O *__restrict__ out) {
  const int img = blockIdx.y, si = img / a.views, v = img - si * a.views;
  const unsigned item = blockIdx.x * kBlock + threadIdx.x;
  const int y = (int)(item / (unsigned)a.runs);
  if (y >= a.Hp) return;
  const int x0 = (int)(item - (unsigned)y * (unsigned)a.runs) * kRun;
  const S *__restrict__ src = (const S *)a.s[si].data;
  const int h = a.s[si].h, w = a.s[si].w;
  // pixels of this run that lie inside the image (0 .. kRun); the others are padding
  int nvalid = 0;
  if (y < h && x0 < w) nvalid = w - x0 < kRun ? w - x0 : kRun;
  const int nstore = a.Wp - x0 < kRun ? a.Wp - x0 : kRun;  // >= 1; kRun whenever out_vec
  const bool vec = a.out_vec != 0;

  float val[3][kRun];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (nvalid > 0) {
      const int cs = a.swap ? 2 - c : c;
      load_run(src + ((size_t)(v * 3 + cs) * h + y) * w + x0, nvalid, val[c]);
    }
    const float m = a.mean[c], sd = a.std[c];
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
      float r = a.pad;
      if (j < nvalid) r = a.normalise ? (val[c][j] - m) / sd : val[c][j];
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

template <typename S, typename O>
void launch(const Args &a, int images, int pixel_major, void *out, hipStream_t s) {
  const dim3 grid(ceil_div((long long)a.Hp * a.runs, kBlock), images);
  if (pixel_major)
    hipLaunchKernelGGL((img_preprocess_kernel<S, O, true>), grid, dim3(kBlock), 0, s, a, (O *)out);
  else
    hipLaunchKernelGGL((img_preprocess_kernel<S, O, false>), grid, dim3(kBlock), 0, s, a, (O *)out);
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_img_preprocess_max_samples(void) { return kMaxSamples; }

BFHIP_EXPORT int bfhip_img_preprocess(const bfhip_img_desc *samples_host, int n_samples, int views, int src_dtype, int swap_rb,
                                      int normalise, const float *mean_host, const float *std_host, float pad_value, int Hp,
                                      int Wp, int out_dtype, int pixel_major, void *out, void *stream) {
  BFHIP_REQUIRE(samples_host && out, "img_preprocess: samples_host and out are required");
  BFHIP_REQUIRE(n_samples >= 1 && views >= 1 && views <= kMaxViews, "img_preprocess: n_samples=%d views=%d (views <= %d)",
                n_samples, views, kMaxViews);
  BFHIP_REQUIRE(src_dtype == 0 || src_dtype == 1, "img_preprocess: src_dtype %d (0 = uint8, 1 = float32)", src_dtype);
  BFHIP_REQUIRE(out_dtype == 0 || out_dtype == 1, "img_preprocess: out_dtype %d (0 = float32, 1 = bf16)", out_dtype);
  BFHIP_REQUIRE(!normalise || (mean_host && std_host), "img_preprocess: normalise needs mean_host and std_host");
  BFHIP_REQUIRE(Hp >= 1 && Wp >= 1 && (long long)Hp * ((Wp + kRun - 1) / kRun) <= 0x7fffffffll,
                "img_preprocess: padded size %d x %d", Hp, Wp);
  for (int i = 0; i < n_samples; ++i) {
    const bfhip_img_desc &d = samples_host[i];
    BFHIP_REQUIRE(d.data && d.h >= 1 && d.w >= 1, "img_preprocess: sample %d: data=%p h=%d w=%d", i, d.data, d.h, d.w);
    BFHIP_REQUIRE(d.h <= Hp && d.w <= Wp, "img_preprocess: sample %d is %d x %d, larger than the padded %d x %d", i, d.h, d.w,
                  Hp, Wp);
  }
  Args a;
  for (int c = 0; c < 3; ++c) {
    a.mean[c] = normalise ? mean_host[c] : 0.f;
    a.std[c] = normalise ? std_host[c] : 1.f;
  }
  a.pad = pad_value;
  a.views = views;
  a.Hp = Hp;
  a.Wp = Wp;
  a.runs = (Wp + kRun - 1) / kRun;
  a.swap = swap_rb ? 1 : 0;
  a.normalise = normalise ? 1 : 0;
  const size_t sample_bytes = (size_t)views * 3 * Hp * Wp * (out_dtype == 1 ? 2 : 4);
  for (int first = 0; first < n_samples; first += kMaxSamples) {
    const int n = n_samples - first < kMaxSamples ? n_samples - first : kMaxSamples;
    for (int i = 0; i < kMaxSamples; ++i) a.s[i] = samples_host[first + (i < n ? i : 0)];
    char *dst = (char *)out + (size_t)first * sample_bytes;
    a.out_vec = (Wp % kRun == 0 && ((uintptr_t)dst & 15) == 0) ? 1 : 0;
    if (src_dtype == 0) {
      if (out_dtype == 1) launch<uint8_t, bf16_t>(a, n * views, pixel_major, dst, (hipStream_t)stream);
      else launch<uint8_t, float>(a, n * views, pixel_major, dst, (hipStream_t)stream);
    } else {
      if (out_dtype == 1) launch<float, bf16_t>(a, n * views, pixel_major, dst, (hipStream_t)stream);
      else launch<float, float>(a, n * views, pixel_major, dst, (hipStream_t)stream);
    }
    const int rc = check_launch("img_preprocess");
    if (rc != BFHIP_OK) return rc;
  }
  return BFHIP_OK;
}
