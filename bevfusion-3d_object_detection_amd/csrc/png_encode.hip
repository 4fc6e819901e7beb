// png_encode.hip -- lossless PNG encode of a batch of RGB frames in four launches, whatever the number of frames and bands:
//   1. png_filter_kernel   one workgroup a row: the five filters' costs, the choice, the filtered row into the workspace
//   2. png_band_kernel     one workgroup a band: run tokens -> symbol histogram (integer LDS adds) and Adler sums; the 15-bit
//                          length-limited code (rank sort in parallel, package-merge on one thread) and its canonical codes;
//                          the stored / dynamic decision; then the band's bytes into its slab of the workspace -- header and
//                          token bits OR-ed at offsets from a workgroup scan into words the kernel zeroed, or a plain copy
//   3. png_offsets_kernel  one workgroup a frame: scan of the bands' byte lengths, the frame's result words
//   4. png_compact_kernel  one workgroup a band: the slab to its place in the frame's stream, nothing at or past the capacity
// bfhip_png_deflate runs 2 - 4 over bytes already on the device.  The format, the capacity bound and every helper the kernels
// share with the host path are in csrc/png_encode_host.h; bevfusion_amd/png_encode.py defines the bytes.
#include "common.h"
#include "png_encode_host.h"

namespace bfhip {

typedef uint32_t U;
typedef unsigned long long U64;

constexpr int kPngThreads = 256;
constexpr int kPngPerThread = 8;                          // consecutive bytes a thread walks
constexpr int kPngTile = kPngThreads * kPngPerThread;     // bytes a workgroup takes per round
constexpr int kPngRecordWords = 8;                        // per band: bytes, stored, Adler A, B, n, longest code, begin lo, hi

// a job's part of the workspace: the band records, the bands' slabs, the filtered bytes (encode only)
struct PngLayout {
  long long n_bands;
  size_t slab_at, slab_stride, filt_at, total;
};

__host__ __device__ inline PngLayout png_layout(long long n_bytes, long long band_bytes, bool with_filter) {
  PngLayout l;
  l.n_bands = bfpng::band_count(n_bytes, band_bytes);
  l.slab_at = ((size_t)l.n_bands * kPngRecordWords * 4 + 255) / 256 * 256;
  const long long longest = band_bytes < n_bytes ? band_bytes : n_bytes;
  l.slab_stride = ((size_t)bfpng::stored_bytes(longest) + 8 + 15) / 16 * 16;  // a dynamic band is shorter than its stored form
  l.filt_at = (l.slab_at + l.slab_stride * (size_t)l.n_bands + 255) / 256 * 256;
  l.total = with_filter ? (l.filt_at + (size_t)n_bytes + 255) / 256 * 256 : l.filt_at;
  return l;
}

// exclusive scan of one value a thread over the workgroup; *total: the sum.  sums: kPngThreads / 64 values of LDS.
template <typename T>
__device__ __forceinline__ T png_exclusive_scan(T x, T *sums, T *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  __syncthreads();  // the previous use of sums is over
  if (lane == 63) sums[wave] = incl;
  __syncthreads();
  T before = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < kPngThreads / 64; ++k) {
    const T s = sums[k];
    if (k < wave) before += s;
    sum += s;
  }
  *total = sum;
  return before + incl - x;
}

// the largest x of the threads before this one (-1: none); *total: the largest of all
__device__ __forceinline__ int png_exclusive_max(int x, int *sums, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d, 64);
    if (lane >= d) incl = max(incl, up);
  }
  int excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = -1;
  __syncthreads();
  if (lane == 63) sums[wave] = incl;
  __syncthreads();
  int all = -1;
#pragma unroll
  for (int k = 0; k < kPngThreads / 64; ++k) {
    const int s = sums[k];
    if (k < wave) excl = max(excl, s);
    all = max(all, s);
  }
  *total = all;
  return excl;
}

__device__ __forceinline__ U64 png_block_sum(U64 x, U64 *sums) {
  U64 total;
  png_exclusive_scan<U64>(x, sums, &total);
  return total;
}

// ------------------------------------------------------------------------------------------------ the filter
// grid (most rows of a frame, n_frames)
__global__ __launch_bounds__(kPngThreads) void png_filter_kernel(const bfhip_png_frame *__restrict__ frames,
                                                                const uint8_t *__restrict__ rgb, uint8_t *__restrict__ workspace) {
  __shared__ U wave_cost[kPngThreads / 64][5];
  const bfhip_png_frame &f = frames[blockIdx.y];
  const int row = blockIdx.x;
  if (row >= f.height) return;
  const int tid = threadIdx.x, rb = 3 * f.width;
  const uint8_t *cur = rgb + f.src_off + (long long)row * rb;
  const uint8_t *up = cur - rb;
  const bool has_up = row > 0;
  U cost[5] = {0, 0, 0, 0, 0};
  for (int i = tid; i < rb; i += kPngThreads) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = has_up ? up[i] : 0, c = has_up && i >= 3 ? up[i - 3] : 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) cost[t] += (U)bfpng::filter_cost(bfpng::filter_byte(t, x, a, b, c));
  }
#pragma unroll
  for (int t = 0; t < 5; ++t) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cost[t] += __shfl_down(cost[t], d, 64);
    if ((tid & 63) == 0) wave_cost[tid >> 6][t] = cost[t];
  }
  __syncthreads();
  int type = 0;
  U best = 0;
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    U sum = 0;
#pragma unroll
    for (int k = 0; k < kPngThreads / 64; ++k) sum += wave_cost[k][t];
    if (t == 0 || sum < best) { best = sum; type = t; }
  }
  const PngLayout lay = png_layout(f.n_bytes, f.band_bytes, true);
  uint8_t *dst = workspace + f.ws_off + lay.filt_at + (long long)row * (rb + 1);
  if (tid == 0) dst[0] = (uint8_t)type;
  for (int i = tid; i < rb; i += kPngThreads) {
    const int x = cur[i], a = i >= 3 ? cur[i - 3] : 0, b = has_up ? up[i] : 0, c = has_up && i >= 3 ? up[i - 3] : 0;
    dst[1 + i] = (uint8_t)bfpng::filter_byte(type, x, a, b, c);
  }
}

// ------------------------------------------------------------------------------------------------ the bands
struct PngShared {
  uint8_t tile[kPngTile + 8];  // [0]: the byte before the round's first, [1 .. kPngTile]: the round's, then the one after
  U hist[bfpng::kSymbols];
  U codes[bfpng::kSymbols];    // bit-reversed code << 8 | length
  uint8_t lens[bfpng::kSymbols + 2];
  U count[16], next_code[16];
  U64 sums64[kPngThreads / 64];
  U sums32[kPngThreads / 64];
  int sums_max[kPngThreads / 64];
  int n_used, max_len;
  bfpng::HuffScratch hs;
};

// OR `len` <= 32 bits of v into the zeroed slab at bit `at`, LSB first
__device__ __forceinline__ void png_or_bits(U *slab, U at, U v, int len) {
  const U64 wide = (U64)v << (at & 31);
  atomicOr(slab + at / 32, (U)wide);
  if ((at & 31) + len > 32) atomicOr(slab + at / 32 + 1, (U)(wide >> 32));
}

// A thread's bit writer, LSB first: whole words, the first one sharing its low bits with the thread before
struct PngBitWriter {
  U *word;
  U64 acc;  // the low n bits are pending
  int n;
  __device__ __forceinline__ void put(U v, int len) {  // len <= 16
    acc |= (U64)v << n;
    n += len;
    if (n >= 32) {
      atomicOr(word++, (U)acc);
      acc >>= 32;
      n -= 32;
    }
  }
  __device__ __forceinline__ void code(U e) { put(e >> 8, (int)(e & 255u)); }
  __device__ __forceinline__ void finish() {
    if (n) atomicOr(word, (U)acc);
  }
};

// One walk over the band, kPngTile bytes a round.  A thread finds the stretches that END in its kPngPerThread bytes (their
// start comes from a max-scan of the run starts, carried from round to round) and handles each whole: EMIT false adds its
// tokens to the histogram and the bytes to the Adler sums; EMIT true sizes them, scans, and writes their bits from bit `at` on.
template <bool EMIT>
__device__ __forceinline__ void png_band_pass(PngShared &sh, const uint8_t *__restrict__ src, long long nb, U *slab, U at, U64 *s1,
                                              U64 *s2) {
  const int tid = threadIdx.x, l0 = tid * kPngPerThread;
  long long carry = 0;  // where the stretch that is open at the round's first byte began
  for (long long base = 0; base < nb; base += kPngTile) {
    __syncthreads();  // the round before has read its tile
    for (int j = tid; j < kPngTile + 2; j += kPngThreads) {
      const long long p = base - 1 + j;
      sh.tile[j] = p >= 0 && p < nb ? src[p] : (uint8_t)0;
    }
    __syncthreads();
    int last = -1;
#pragma unroll
    for (int k = 0; k < kPngPerThread; ++k) {
      const long long p = base + l0 + k;
      if (p < nb && (p == 0 || sh.tile[l0 + k + 1] != sh.tile[l0 + k])) last = l0 + k;
    }
    int tile_last;
    const int before = png_exclusive_max(last, sh.sums_max, &tile_last);
    const long long open = before >= 0 ? base + before : carry;
    long long s = open;
    U bits = 0;
    for (int k = 0; k < kPngPerThread; ++k) {
      const long long p = base + l0 + k;
      if (p >= nb) break;
      const int x = sh.tile[l0 + k + 1];
      if (p == 0 || x != sh.tile[l0 + k]) s = p;
      if (!EMIT) {
        *s1 += (U64)x;
        *s2 += (U64)(nb - p) * (U64)x;
      }
      if (p != nb - 1 && sh.tile[l0 + k + 2] == x) continue;
      const bfpng::RunPlan plan = bfpng::plan_run(p - s + 1);
      int sym = 0, ne = 0, ex = 0;
      if (plan.rem >= 3) bfpng::length_symbol(plan.rem, &sym, &ne, &ex);
      if (!EMIT) {
        atomicAdd(&sh.hist[x], (U)(1 + (plan.rem < 3 ? plan.rem : 0)));
        if (plan.q) atomicAdd(&sh.hist[285], (U)plan.q);
        if (plan.rem >= 3) atomicAdd(&sh.hist[sym], 1u);
      } else {
        const U lit = sh.codes[x] & 255u;
        bits += lit * (U)(1 + (plan.rem < 3 ? plan.rem : 0)) + (U)plan.q * ((sh.codes[285] & 255u) + 1u);
        if (plan.rem >= 3) bits += (sh.codes[sym] & 255u) + (U)ne + 1u;
        if (p == nb - 1) bits += sh.codes[bfpng::kEob] & 255u;
      }
    }
    if (EMIT) {
      U round_bits;
      const U mine = at + png_exclusive_scan<U>(bits, sh.sums32, &round_bits);
      PngBitWriter bw = {slab + mine / 32, 0, (int)(mine & 31)};
      s = open;
      for (int k = 0; k < kPngPerThread; ++k) {
        const long long p = base + l0 + k;
        if (p >= nb) break;
        const int x = sh.tile[l0 + k + 1];
        if (p == 0 || x != sh.tile[l0 + k]) s = p;
        if (p != nb - 1 && sh.tile[l0 + k + 2] == x) continue;
        const bfpng::RunPlan plan = bfpng::plan_run(p - s + 1);
        const U lit = sh.codes[x], far = sh.codes[285];
        bw.code(lit);
        for (long long m = 0; m < plan.q; ++m) {
          bw.code(far);
          bw.put(0, 1);
        }
        if (plan.rem >= 3) {
          int sym, ne, ex;
          bfpng::length_symbol(plan.rem, &sym, &ne, &ex);
          bw.code(sh.codes[sym]);
          if (ne) bw.put((U)ex, ne);
          bw.put(0, 1);
        } else {
          for (int m = 0; m < plan.rem; ++m) bw.code(lit);
        }
        if (p == nb - 1) bw.code(sh.codes[bfpng::kEob]);
      }
      bw.finish();
      at += round_bits;
    }
    if (tile_last >= 0) carry = base + tile_last;
  }
}

// grid (most bands of a job, n_jobs).  data: the bytes (deflate), or null: the job's filtered bytes in the workspace.
__global__ __launch_bounds__(kPngThreads) void png_band_kernel(const bfhip_png_frame *__restrict__ frames,
                                                              const uint8_t *__restrict__ data, uint8_t *__restrict__ workspace) {
  __shared__ PngShared sh;
  const bfhip_png_frame &f = frames[blockIdx.y];
  const bool with_filter = data == nullptr;
  const PngLayout lay = png_layout(f.n_bytes, f.band_bytes, with_filter);
  const long long b = blockIdx.x;
  if (b >= lay.n_bands) return;
  const int tid = threadIdx.x;
  uint8_t *ws = workspace + f.ws_off;
  const uint8_t *src = (with_filter ? ws + lay.filt_at : data + f.src_off) + b * f.band_bytes;
  const long long left = f.n_bytes - b * f.band_bytes, nb = left < f.band_bytes ? left : f.band_bytes;
  const bool final = b == lay.n_bands - 1;
  uint8_t *slab8 = ws + lay.slab_at + lay.slab_stride * (size_t)b;
  U *slab = reinterpret_cast<U *>(slab8);
  for (int t = tid; t < bfpng::kSymbols; t += kPngThreads) {
    sh.hist[t] = t == bfpng::kEob ? 1u : 0u;
    sh.lens[t] = 0;
  }
  if (tid < 16) sh.count[tid] = 0;
  if (tid == 0) { sh.n_used = 0; sh.max_len = 0; }
  U64 s1 = 0, s2 = 0;
  png_band_pass<false>(sh, src, nb, slab, 0, &s1, &s2);  // begins with a barrier
  __syncthreads();
  s1 = png_block_sum(s1, sh.sums64);
  s2 = png_block_sum(s2, sh.sums64);
  // the used symbols in ascending order of (count, symbol)
  for (int t = tid; t < bfpng::kSymbols; t += kPngThreads) {
    const U h = sh.hist[t];
    if (!h) continue;
    int r = 0;
    for (int j = 0; j < bfpng::kSymbols; ++j) {
      const U hj = sh.hist[j];
      r += hj && (hj < h || (hj == h && j < t)) ? 1 : 0;
    }
    sh.hs.w[r] = h;
    sh.hs.sym[r] = (uint16_t)t;
    atomicAdd(&sh.n_used, 1);
  }
  __syncthreads();
  const int n = sh.n_used;  // >= 2: a literal and end-of-block
  if (tid == 0) bfpng::package_merge(&sh.hs, n, bfpng::kMaxLen);
  __syncthreads();
  for (int r = tid; r < n; r += kPngThreads) {
    const int len = bfpng::rank_length(&sh.hs, r, bfpng::kMaxLen);
    sh.lens[sh.hs.sym[r]] = (uint8_t)len;
    atomicAdd(&sh.count[len], 1u);
    atomicMax(&sh.max_len, len);
  }
  __syncthreads();
  if (tid == 0) {
    U code = 0;
    sh.next_code[0] = 0;
    for (int k = 1; k <= bfpng::kMaxLen; ++k) {
      code = (code + (k > 1 ? sh.count[k - 1] : 0u)) << 1;
      sh.next_code[k] = code;
    }
  }
  __syncthreads();
  U64 my_bits = 0, my_matches = 0;
  for (int t = tid; t < bfpng::kSymbols; t += kPngThreads) {
    const int len = sh.lens[t];
    U e = 0;
    if (len) {
      U c = sh.next_code[len];
      for (int j = 0; j < t; ++j) c += sh.lens[j] == len ? 1u : 0u;
      e = ((__brev(c) >> (32 - len)) << 8) | (U)len;
    }
    sh.codes[t] = e;
    my_bits += (U64)sh.hist[t] * (U64)(len + (t > bfpng::kEob ? bfpng::length_extra_bits(t) : 0));
    if (t > bfpng::kEob) my_matches += sh.hist[t];
  }
  const U64 matches = png_block_sum(my_matches, sh.sums64);
  const U64 bits = bfpng::kHeaderBits + matches + png_block_sum(my_bits, sh.sums64);  // the codes are in LDS after these barriers
  const U64 dyn_bytes = final ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
  const bool stored = dyn_bytes >= (U64)bfpng::stored_bytes(nb);
  U64 bytes;
  if (stored) {
    bytes = (U64)bfpng::stored_bytes(nb);
    for (long long i = tid; i < nb; i += kPngThreads) slab8[5 * (i / 65535 + 1) + i] = src[i];
    const long long chunks = (nb + 65534) / 65535;
    for (long long c = tid; c < chunks; c += kPngThreads) {
      const long long rest = nb - c * 65535;
      const U len = (U)(rest < 65535 ? rest : 65535);
      uint8_t *h = slab8 + c * 65540;
      h[0] = final && c == chunks - 1 ? 1 : 0;
      h[1] = (uint8_t)len; h[2] = (uint8_t)(len >> 8); h[3] = (uint8_t)~len; h[4] = (uint8_t)(~len >> 8);
    }
  } else {
    bytes = dyn_bytes;
    for (U64 w = tid; w < (dyn_bytes + 3) / 4; w += kPngThreads) slab[w] = 0;
    __syncthreads();
    if (tid == 0) {
      PngBitWriter bw = {slab, 0, 0};
      bw.put(final ? 1u : 0u, 1);
      bw.put(2, 2);
      bw.put(29, 5);
      bw.put(0, 5);
      bw.put(15, 4);
      bw.put(0, 9);  // code-length symbols 16, 17, 18: no code
      for (int k = 0; k < 16; ++k) bw.put(4, 3);
      bw.finish();
      png_or_bits(slab, bfpng::kPrefixBits + 4 * bfpng::kSymbols, matches ? 8u : 0u, 4);  // length 1, reversed on four bits
      if (!final) {
        const U64 o = (bits + 3 + 7) / 8 + 2;  // 00 00 FF FF
        atomicOr(slab + o / 4, 0xFFu << (8 * (o & 3)));
        atomicOr(slab + (o + 1) / 4, 0xFFu << (8 * ((o + 1) & 3)));
      }
    }
    for (int t = tid; t < bfpng::kSymbols; t += kPngThreads)
      png_or_bits(slab, (U)(bfpng::kPrefixBits + 4 * t), __brev((U)sh.lens[t]) >> 28, 4);
    png_band_pass<true>(sh, src, nb, slab, (U)bfpng::kHeaderBits, &s1, &s2);
  }
  if (tid == 0) {
    U *rec = reinterpret_cast<U *>(ws) + kPngRecordWords * b;
    rec[0] = (U)bytes;
    rec[1] = stored ? 1u : 0u;
    rec[2] = (U)((1 + s1) % bfpng::kAdlerMod);
    rec[3] = (U)(((U64)nb + s2) % bfpng::kAdlerMod);
    rec[4] = (U)nb;
    rec[5] = (U)sh.max_len;
  }
}

// grid (n_jobs): where every band begins in the stream, and the job's result words
__global__ __launch_bounds__(kPngThreads) void png_offsets_kernel(const bfhip_png_frame *__restrict__ frames, uint8_t *__restrict__ workspace,
                                                                 U *__restrict__ result, int with_filter) {
  __shared__ U64 sums64[kPngThreads / 64];
  __shared__ int max_len;
  const bfhip_png_frame &f = frames[blockIdx.x];
  const PngLayout lay = png_layout(f.n_bytes, f.band_bytes, with_filter != 0);
  const int tid = threadIdx.x;
  U *recs = reinterpret_cast<U *>(workspace + f.ws_off);
  U *res = result + f.res_off;
  if (tid == 0) max_len = 0;
  U64 running = 2, my_stored = 0;
  int my_max = 0;
  for (long long base = 0; base < lay.n_bands; base += kPngThreads) {
    const long long k = base + tid;
    const bool live = k < lay.n_bands;
    U *rec = recs + kPngRecordWords * (live ? k : 0);
    const U64 bytes = live ? rec[0] : 0;
    U64 round;
    const U64 begin = running + png_exclusive_scan<U64>(bytes, sums64, &round);
    if (live) {
      rec[6] = (U)begin;
      rec[7] = (U)(begin >> 32);
      U *band = res + bfpng::kResultWords + bfpng::kBandWords * k;
      band[0] = rec[2]; band[1] = rec[3]; band[2] = rec[4]; band[3] = rec[0] | (rec[1] << 31);
      my_stored += rec[1];
      my_max = max(my_max, (int)rec[5]);
    }
    running += round;
  }
  const U64 stored = png_block_sum(my_stored, sums64);
  atomicMax(&max_len, my_max);
  __syncthreads();
  if (tid == 0) {
    res[0] = (U)running;
    res[1] = (U)(running >> 32);
    res[2] = running > (U64)f.capacity ? BFHIP_PNG_OVERFLOW : 0;
    res[3] = (U)stored;
    res[4] = (U)((U64)lay.n_bands - stored);
    res[5] = (U)max_len;
    res[6] = (U)lay.n_bands;
    res[7] = 0;
  }
}

// grid (most bands of a job, n_jobs)
__global__ __launch_bounds__(kPngThreads) void png_compact_kernel(const bfhip_png_frame *__restrict__ frames,
                                                                 const uint8_t *__restrict__ workspace, uint8_t *__restrict__ out,
                                                                 int with_filter) {
  const bfhip_png_frame &f = frames[blockIdx.y];
  const PngLayout lay = png_layout(f.n_bytes, f.band_bytes, with_filter != 0);
  const long long b = blockIdx.x;
  if (b >= lay.n_bands) return;
  const int tid = threadIdx.x;
  const uint8_t *ws = workspace + f.ws_off;
  const U *rec = reinterpret_cast<const U *>(ws) + kPngRecordWords * b;
  const uint8_t *slab8 = ws + lay.slab_at + lay.slab_stride * (size_t)b;
  const long long begin = (long long)((U64)rec[6] | ((U64)rec[7] << 32)), bytes = rec[0], cap = f.capacity;
  uint8_t *dst = out + f.out_off;
  if (b == 0 && tid == 0) {
    if (cap > 0) dst[0] = 0x78;
    if (cap > 1) dst[1] = 0x01;
  }
  for (long long i = tid; i < bytes; i += kPngThreads)
    if (begin + i < cap) dst[begin + i] = slab8[i];
}

// Validates the host copy of the table; encode: the pixels and the geometry too.
static int png_validate(const char *who, const bfhip_png_frame *frames, int n, bool encode, size_t src_bytes, size_t workspace_bytes,
                        size_t out_bytes, size_t result_words, long long *most_bands, int *most_rows) {
  BFHIP_REQUIRE(n >= 1 && n <= 65535, "%s: %d jobs outside 1..65535", who, n);
  long long out_end = 0, ws_end = 0, res_end = 0;
  *most_bands = 0;
  *most_rows = 0;
  for (int i = 0; i < n; ++i) {
    const bfhip_png_frame &f = frames[i];
    BFHIP_REQUIRE(f.n_bytes >= 1 && f.n_bytes <= bfpng::kMaxBytes && f.band_bytes >= 1 && f.band_bytes <= bfpng::kMaxBandBytes,
                  "%s: job %d: %lld bytes in bands of %lld", who, i, (long long)f.n_bytes, (long long)f.band_bytes);
    if (encode) {
      BFHIP_REQUIRE(f.width >= 1 && f.height >= 1 && f.width <= 65535 && f.height <= 65535, "%s: frame %d: %dx%d", who, i, f.width, f.height);
      const long long row = 1 + 3ll * f.width;
      BFHIP_REQUIRE(f.n_bytes == row * f.height && f.band_bytes % row == 0,
                    "%s: frame %d: n_bytes is not height (1 + 3 width) or a band is not whole rows", who, i);
      BFHIP_REQUIRE(f.src_off >= 0 && (unsigned long long)(f.src_off + 3ll * f.width * f.height) <= src_bytes,
                    "%s: frame %d: pixels outside the input block", who, i);
    } else {
      BFHIP_REQUIRE(f.src_off >= 0 && (unsigned long long)(f.src_off + f.n_bytes) <= src_bytes, "%s: job %d: bytes outside the input block", who, i);
    }
    const PngLayout lay = png_layout(f.n_bytes, f.band_bytes, encode);
    const long long words = bfpng::kResultWords + bfpng::kBandWords * lay.n_bands;
    BFHIP_REQUIRE(f.capacity >= 0 && f.out_off >= out_end && (unsigned long long)(f.out_off + f.capacity) <= out_bytes,
                  "%s: job %d: its output overlaps the job before or leaves the buffer", who, i);
    BFHIP_REQUIRE(f.ws_off >= ws_end && f.ws_off % 256 == 0 && (unsigned long long)f.ws_off + lay.total <= workspace_bytes,
                  "%s: job %d: its workspace overlaps the job before or leaves the buffer", who, i);
    BFHIP_REQUIRE(f.res_off >= res_end && (unsigned long long)(f.res_off + words) <= result_words,
                  "%s: job %d: its result words overlap the job before or leave the buffer", who, i);
    out_end = f.out_off + f.capacity;
    ws_end = f.ws_off + (long long)lay.total;
    res_end = f.res_off + words;
    *most_bands = lay.n_bands > *most_bands ? lay.n_bands : *most_bands;
    *most_rows = f.height > *most_rows ? f.height : *most_rows;
  }
  BFHIP_REQUIRE(*most_bands <= 0x7fffffffll, "%s: %lld bands in one job", who, *most_bands);
  return BFHIP_OK;
}

static int png_launch(const bfhip_png_frame *frames_dev, int n, long long most_bands, int most_rows, const uint8_t *src_dev, bool encode,
                      uint8_t *workspace, uint8_t *out_dev, U *result_dev, hipStream_t s) {
  int rc;
  if (encode) {
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)most_rows, (unsigned)n), dim3(kPngThreads), 0, s, frames_dev, src_dev, workspace);
    if ((rc = check_launch("png_filter_kernel"))) return rc;
  }
  hipLaunchKernelGGL(png_band_kernel, dim3((unsigned)most_bands, (unsigned)n), dim3(kPngThreads), 0, s, frames_dev,
                     encode ? (const uint8_t *)nullptr : src_dev, workspace);
  if ((rc = check_launch("png_band_kernel"))) return rc;
  hipLaunchKernelGGL(png_offsets_kernel, dim3((unsigned)n), dim3(kPngThreads), 0, s, frames_dev, workspace, result_dev, encode ? 1 : 0);
  if ((rc = check_launch("png_offsets_kernel"))) return rc;
  hipLaunchKernelGGL(png_compact_kernel, dim3((unsigned)most_bands, (unsigned)n), dim3(kPngThreads), 0, s, frames_dev, workspace, out_dev,
                     encode ? 1 : 0);
  return check_launch("png_compact_kernel");
}

static int png_run(const char *who, bool encode, const bfhip_png_frame *frames_host, const bfhip_png_frame *frames_dev, int n,
                   const uint8_t *src_dev, size_t src_bytes, void *workspace, size_t workspace_bytes, uint8_t *out_dev, size_t out_bytes,
                   uint32_t *result_dev, size_t result_words, void *stream) {
  BFHIP_REQUIRE(frames_host && frames_dev && src_dev && workspace && out_dev && result_dev, "%s: null argument", who);
  BFHIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(result_dev) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(frames_dev) & 7) == 0,
                "%s: the workspace must be 256-byte, the table 8-byte and result_dev 4-byte aligned", who);
  long long most_bands;
  int most_rows;
  const int rc = png_validate(who, frames_host, n, encode, src_bytes, workspace_bytes, out_bytes, result_words, &most_bands, &most_rows);
  if (rc) return rc;
  return png_launch(frames_dev, n, most_bands, most_rows, src_dev, encode, (uint8_t *)workspace, out_dev, result_dev, (hipStream_t)stream);
}

static bool png_sizes_ok(int64_t n_bytes, int64_t band_bytes) {
  return n_bytes >= 1 && n_bytes <= bfpng::kMaxBytes && band_bytes >= 1 && band_bytes <= bfpng::kMaxBandBytes;
}

}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_png_encode_supported(int width, int height, int band_rows) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || band_rows < 1) return 0;
  const long long row = 1 + 3ll * width;
  return png_sizes_ok(row * height, row * (band_rows < height ? band_rows : height)) ? 1 : 0;
}

BFHIP_EXPORT int bfhip_png_encode_max_frames(void) { return 65535; }

BFHIP_EXPORT size_t bfhip_png_workspace_bytes(int64_t n_bytes, int64_t band_bytes, int with_filter) {
  return png_sizes_ok(n_bytes, band_bytes) ? png_layout(n_bytes, band_bytes, with_filter != 0).total : 0;
}

BFHIP_EXPORT size_t bfhip_png_capacity(int64_t n_bytes, int64_t band_bytes) {
  return png_sizes_ok(n_bytes, band_bytes) ? (size_t)bfpng::capacity(n_bytes, band_bytes) : 0;
}

BFHIP_EXPORT size_t bfhip_png_result_words(int64_t n_bytes, int64_t band_bytes) {
  return png_sizes_ok(n_bytes, band_bytes) ? (size_t)(bfpng::kResultWords + bfpng::kBandWords * bfpng::band_count(n_bytes, band_bytes)) : 0;
}

BFHIP_EXPORT int bfhip_png_encode(const bfhip_png_frame *frames_host, const bfhip_png_frame *frames_dev, int n_frames,
                                  const uint8_t *rgb_dev, size_t rgb_bytes, void *workspace, size_t workspace_bytes, uint8_t *out_dev,
                                  size_t out_bytes, uint32_t *result_dev, size_t result_words, void *stream) {
  return png_run("bfhip_png_encode", true, frames_host, frames_dev, n_frames, rgb_dev, rgb_bytes, workspace, workspace_bytes, out_dev,
                 out_bytes, result_dev, result_words, stream);
}

BFHIP_EXPORT int bfhip_png_deflate(const bfhip_png_frame *jobs_host, const bfhip_png_frame *jobs_dev, int n_jobs, const uint8_t *data_dev,
                                   size_t data_bytes, void *workspace, size_t workspace_bytes, uint8_t *out_dev, size_t out_bytes,
                                   uint32_t *result_dev, size_t result_words, void *stream) {
  return png_run("bfhip_png_deflate", false, jobs_host, jobs_dev, n_jobs, data_dev, data_bytes, workspace, workspace_bytes, out_dev,
                 out_bytes, result_dev, result_words, stream);
}

BFHIP_EXPORT int bfhip_png_filter_host(const uint8_t *rgb, int width, int height, uint8_t *out, size_t out_bytes) {
  char err[bfpng::kErrLen];
  const int rc = bfpng::filter_rows(rgb, width, height, out, out_bytes, err);
  if (rc) set_error("%s", err);
  return rc;
}

BFHIP_EXPORT int bfhip_png_huffman_lengths(const uint32_t *hist, int n_symbols, int max_len, uint8_t *lens) {
  char err[bfpng::kErrLen];
  const int rc = bfpng::huffman_lengths(hist, n_symbols, max_len, lens, err);
  if (rc) set_error("%s", err);
  return rc;
}

BFHIP_EXPORT int bfhip_png_deflate_host(const uint8_t *data, size_t n, size_t band_bytes, uint8_t *out, size_t capacity, uint32_t *bands,
                                        size_t band_slots, bfhip_png_stats *stats) {
  char err[bfpng::kErrLen];
  const int rc = bfpng::deflate_rle(data, n, band_bytes, out, capacity, bands, band_slots, stats, err);
  if (rc) set_error("%s", err);
  return rc;
}
