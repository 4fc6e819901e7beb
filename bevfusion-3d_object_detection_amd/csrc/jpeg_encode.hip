// jpeg_encode.hip -- baseline JPEG encode of a batch of RGB frames in three launches, the decoder (csrc/jpeg.hip) turned round:
//   1. jpeg_forward_kernel  colour conversion, edge padding, chroma downsampling, libjpeg's accurate integer forward DCT
//                           (jfdctint), quantisation and the dummy blocks -> int16 coefficients in the decoder's layout
//   2. jpeg_huffman_kernel  one workgroup per MCU row (= restart interval): every thread codes whole blocks, a workgroup scan
//                           gives their bit offsets, the bits go into the interval's slab of the workspace
//   3. jpeg_compact_kernel  one workgroup per interval: FF stuffing, 1-bit padding, RSTm / EOI, into the frame's stream
// The coefficients are defined by bevfusion_amd/jpeg_encode.py (torch_jpeg_forward: 32-bit wrap-around arithmetic, done here on
// uint32_t and cast only for the arithmetic shifts), the bytes by csrc/jpeg_encode_host.h.
#include "common.h"
#include "jpeg_encode_host.h"

namespace bfhip {

typedef uint32_t U;

// One pass of the 8-point forward DCT of libjpeg's jfdctint ("islow", CONST_BITS = 13, PASS1_BITS = 2).  first: outputs 0 and 4
// are shifted left by 2 and the rest descaled by 11; otherwise 0 and 4 are descaled by 2 and the rest by 15.
template <bool first>
__device__ __forceinline__ void fdct_1d(const int32_t *in, int32_t *out) {
  const U d0 = (U)in[0], d1 = (U)in[1], d2 = (U)in[2], d3 = (U)in[3], d4 = (U)in[4], d5 = (U)in[5], d6 = (U)in[6], d7 = (U)in[7];
  const U t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const U t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int shift = first ? 11 : 15;
  const U half = (U)1 << (shift - 1);
  if (first) {
    out[0] = (int32_t)((t10 + t11) << 2);
    out[4] = (int32_t)((t10 - t11) << 2);
  } else {
    out[0] = (int32_t)(t10 + t11 + 2u) >> 2;
    out[4] = (int32_t)(t10 - t11 + 2u) >> 2;
  }
  U z1 = (t12 + t13) * (U)4433;
  out[2] = (int32_t)(z1 + t13 * (U)6270 + half) >> shift;
  out[6] = (int32_t)(z1 + t12 * (U)(-15137) + half) >> shift;
  z1 = t4 + t7;
  U z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const U z5 = (z3 + z4) * (U)9633;
  const U o4 = t4 * (U)2446, o5 = t5 * (U)16819, o6 = t6 * (U)25172, o7 = t7 * (U)12299;
  z1 *= (U)(-7373); z2 *= (U)(-20995); z3 *= (U)(-16069); z4 *= (U)(-3196);
  z3 += z5; z4 += z5;
  out[7] = (int32_t)(o4 + z1 + z3 + half) >> shift;
  out[5] = (int32_t)(o5 + z2 + z4 + half) >> shift;
  out[3] = (int32_t)(o6 + z2 + z3 + half) >> shift;
  out[1] = (int32_t)(o7 + z1 + z4 + half) >> shift;
}

constexpr int kFwdThreads = 256;              // 8 lanes a block
constexpr int kFwdBlocks = kFwdThreads / 8;   // 8x8 blocks a workgroup
constexpr int kFwdStride = 9;                 // int32 row stride of a block's tile: rows and columns both conflict-free

// N pixels of one row from column x0 on; columns past the frame repeat the last one.  A run inside the frame that starts on a
// 4-byte boundary is read as words.
template <int N>
__device__ __forceinline__ void load_pixels(const uint8_t *__restrict__ row, int x0, int W, uint8_t *px) {
  const uint8_t *p = row + (long long)x0 * 3;
  if (x0 + N <= W && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    const U *q = reinterpret_cast<const U *>(p);
#pragma unroll
    for (int j = 0; j < 3 * N / 4; ++j) {
      const U w = q[j];
      px[4 * j] = (uint8_t)w; px[4 * j + 1] = (uint8_t)(w >> 8); px[4 * j + 2] = (uint8_t)(w >> 16); px[4 * j + 3] = (uint8_t)(w >> 24);
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const uint8_t *s = row + (long long)min(x0 + i, W - 1) * 3;
      px[3 * i] = s[0]; px[3 * i + 1] = s[1]; px[3 * i + 2] = s[2];
    }
  }
}

// jccolor's 16-bit fixed-point conversion of one pixel to component c
__device__ __forceinline__ int component(int c, int r, int g, int b) {
  if (c == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (c == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// The 8 samples, less 128, of sample row `sy` of component c from sample column sx0 on, after padding and downsampling.
__device__ __forceinline__ void sample_row(const bfhip_jpeg_enc_frame &f, const uint8_t *__restrict__ rgb, int c, int sx0, int sy,
                                           int32_t *v) {
  const int W = f.width, H = f.height;
  const long long pitch = (long long)W * 3;
  if (c == 0 || f.hs == 1) {  // full resolution
    uint8_t px[24];
    load_pixels<8>(rgb + min(sy, H - 1) * pitch, sx0, W, px);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = component(c, px[3 * i], px[3 * i + 1], px[3 * i + 2]) - 128;
    return;
  }
  uint8_t px[48];
  if (f.vs == 1) {  // h2v1
    load_pixels<16>(rgb + min(sy, H - 1) * pitch, 2 * sx0, W, px);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      v[i] = ((component(c, px[6 * i], px[6 * i + 1], px[6 * i + 2]) + component(c, px[6 * i + 3], px[6 * i + 4], px[6 * i + 5]) +
               (i & 1)) >> 1) - 128;
    return;
  }
  // h2v2: the downsampled plane repeats its last row; the input repeats its last row up to a whole pair
  const int cy = min(sy, (H + 1) / 2 - 1);
  int32_t sum[8];
  load_pixels<16>(rgb + min(2 * cy, H - 1) * pitch, 2 * sx0, W, px);
#pragma unroll
  for (int i = 0; i < 8; ++i)
    sum[i] = component(c, px[6 * i], px[6 * i + 1], px[6 * i + 2]) + component(c, px[6 * i + 3], px[6 * i + 4], px[6 * i + 5]);
  load_pixels<16>(rgb + min(2 * cy + 1, H - 1) * pitch, 2 * sx0, W, px);
#pragma unroll
  for (int i = 0; i < 8; ++i)
    v[i] = ((sum[i] + component(c, px[6 * i], px[6 * i + 1], px[6 * i + 2]) + component(c, px[6 * i + 3], px[6 * i + 4], px[6 * i + 5]) +
             1 + (i & 1)) >> 2) - 128;
}

// grid (ceil(most blocks of a frame / 32), n_frames).  Lane l of a block makes sample row l, runs row l, leaves it in the tile,
// runs column l and quantises it, and after a second turn through the tile stores coefficient row l (one 16-byte store).  A
// dummy luma block transforms the block its DC comes from and keeps the DC alone.
__global__ __launch_bounds__(kFwdThreads) void jpeg_forward_kernel(const bfhip_jpeg_enc_frame *__restrict__ frames,
                                                                  const uint8_t *__restrict__ rgb, int16_t *__restrict__ coef) {
  __shared__ int32_t tile[kFwdBlocks][8 * kFwdStride];
  const bfhip_jpeg_enc_frame &f = frames[blockIdx.y];
  const long long n0 = (long long)f.block_cols[0] * f.block_rows[0], n1 = (long long)f.block_cols[1] * f.block_rows[1];
  const long long total = n0 + n1 + (long long)f.block_cols[2] * f.block_rows[2];
  if ((long long)blockIdx.x * kFwdBlocks >= total) return;  // the whole workgroup: this frame has fewer blocks
  const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
  long long b = (long long)blockIdx.x * kFwdBlocks + slot;
  const bool live = b < total;
  if (!live) b = 0;
  const int c = b < n0 ? 0 : (b < n0 + n1 ? 1 : 2);
  b -= c == 0 ? 0 : (c == 1 ? n0 : n0 + n1);
  const int bc = f.block_cols[c], brow = (int)(b / bc), bcol = (int)(b - (long long)brow * bc);
  int srow = brow, scol = bcol;
  bool dummy = false;
  if (c == 0) {
    const int real_cols = (f.width + 7) >> 3, real_rows = (f.height + 7) >> 3;
    if (brow >= real_rows) { srow = brow - 1; scol = bcol / f.hs * f.hs + f.hs - 1; dummy = true; }
    if (scol >= real_cols) { scol = real_cols - 1; dummy = true; }
  }
  int32_t *t = tile[slot];
  int32_t v[8], w[8];
  if (live) {
    sample_row(f, rgb + f.rgb_off, c, scol * 8, srow * 8 + lane, v);
    fdct_1d<true>(v, w);
#pragma unroll
    for (int x = 0; x < 8; ++x) t[lane * kFwdStride + x] = w[x];
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = t[r * kFwdStride + lane];
    fdct_1d<false>(v, w);
  }
  __syncthreads();
  if (live) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const U qv = (U)f.quant[c][r * 8 + lane] << 3;
      const U ax = (U)(w[r] < 0 ? -w[r] : w[r]);
      const int32_t q = (int32_t)((ax + (qv >> 1)) / qv);
      t[r * kFwdStride + lane] = w[r] < 0 ? -q : q;
    }
  }
  __syncthreads();
  if (live) {
    U pk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int32_t lo = t[lane * kFwdStride + 2 * j], hi = t[lane * kFwdStride + 2 * j + 1];
      if (dummy) { hi = 0; if (lane != 0 || j != 0) lo = 0; }
      pk[j] = ((U)lo & 0xffffu) | ((U)hi << 16);
    }
    *reinterpret_cast<uint4 *>(coef + f.coef_off[c] + b * 64 + lane * 8) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
  }
}

// ------------------------------------------------------------------------------------------------ the Huffman stage
constexpr int kHuffThreads = 256;
constexpr int kSlabWordsPerBlock = bfjpeg_enc::kMaxBlockBits / 32;  // 52 words = 208 bytes: a block's longest code

static __device__ const bfjpeg_enc::Tables kHuffTables = bfjpeg_enc::make_tables();

// natural position -> zigzag position
struct ZigzagOf { uint8_t at[64]; };
constexpr ZigzagOf make_zigzag_of() {
  ZigzagOf z = {};
  for (int k = 0; k < 64; ++k) z.at[bfjpeg_enc::kNatural[k]] = (uint8_t)k;
  return z;
}
static __device__ const ZigzagOf kZigzagOf = make_zigzag_of();

constexpr U kRecordBad = 0x80000000u;  // in an interval's first record word: a coefficient without a code was clamped

// a frame's part of the workspace: per interval {stuffed bytes | kRecordBad, unstuffed bits}, then the slabs
struct EncLayout {
  int mcus_x, mcus_y, blocks_per_mcu;
  long long blocks_per_interval;
  size_t slab_at, slab_bytes_per_interval, total;
};

__host__ __device__ inline EncLayout enc_layout(int width, int height, int hs, int vs) {
  EncLayout l;
  l.mcus_x = (width + 8 * hs - 1) / (8 * hs);
  l.mcus_y = (height + 8 * vs - 1) / (8 * vs);
  l.blocks_per_mcu = hs * vs + 2;
  l.blocks_per_interval = (long long)l.mcus_x * l.blocks_per_mcu;
  l.slab_at = ((size_t)l.mcus_y * 8 + 255) / 256 * 256;
  l.slab_bytes_per_interval = (size_t)l.blocks_per_interval * kSlabWordsPerBlock * 4;
  l.total = (l.slab_at + l.slab_bytes_per_interval * (size_t)l.mcus_y + 255) / 256 * 256;
  return l;
}

// exclusive scan of one value a thread over the workgroup; *total: the sum.  wave_sums: kHuffThreads / 64 + 1 words of LDS.
__device__ __forceinline__ U block_exclusive_scan(U x, U *wave_sums, U *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  U incl = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const U up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  __syncthreads();  // the previous use of wave_sums is over
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  U before = 0, sum = 0;
#pragma unroll
  for (int k = 0; k < kHuffThreads / 64; ++k) {
    const U s = wave_sums[k];
    if (k < wave) before += s;
    sum += s;
  }
  *total = sum;
  return before + incl - x;
}

__device__ __forceinline__ int bit_category(int v) { return 32 - __clz(v < 0 ? -v : v); }

// A thread's bit writer: whole words, the first one sharing its leading bits with the block before, OR-ed into the zeroed slab.
struct BitWriter {
  U *word;       // the next word to complete
  uint64_t acc;  // the low `n` bits are pending
  int n;
  __device__ __forceinline__ void put(U code, int len) {
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      atomicOr(word++, (U)(acc >> (n - 32)));
      n -= 32;
    }
  }
  __device__ __forceinline__ void finish() {
    if (n) atomicOr(word, (U)(acc << (32 - n)));
  }
};

// grid (most MCU rows of a frame, n_frames), one workgroup an interval.  Blocks are taken 256 at a time in scan order; a thread
// keeps its block in LDS in zigzag order ([position][thread], so lanes do not conflict) with a 64-bit mask of the non-zero
// positions, walks the mask once for the length and, after the scan and the zeroing of the words this round completes, once
// more for the bits.
__global__ __launch_bounds__(kHuffThreads) void jpeg_huffman_kernel(const bfhip_jpeg_enc_frame *__restrict__ frames,
                                                                   const int16_t *__restrict__ coef, uint8_t *__restrict__ workspace) {
  __shared__ int16_t zz[64 * kHuffThreads];
  __shared__ U ac_table[2][256];
  __shared__ U dc_table[2][16];
  __shared__ U wave_sums[kHuffThreads / 64 + 1];
  const bfhip_jpeg_enc_frame &f = frames[blockIdx.y];
  const EncLayout lay = enc_layout(f.width, f.height, f.hs, f.vs);
  const int my = blockIdx.x;
  if (my >= lay.mcus_y) return;
  const int tid = threadIdx.x;
  for (int i = tid; i < 512; i += kHuffThreads) ac_table[i >> 8][i & 255] = kHuffTables.ac[i >> 8][i & 255];
  if (tid < 32) dc_table[tid >> 4][tid & 15] = kHuffTables.dc[tid >> 4][tid & 15];
  uint8_t *ws = workspace + f.ws_off;
  U *record = reinterpret_cast<U *>(ws) + 2 * my;
  U *slab = reinterpret_cast<U *>(ws + lay.slab_at + lay.slab_bytes_per_interval * (size_t)my);
  const int luma_blocks = f.hs * f.vs;
  U base_bits = 0;
  bool bad = false;
  for (long long first = 0; first < lay.blocks_per_interval; first += kHuffThreads) {
    const long long i = first + tid;
    const bool live = i < lay.blocks_per_interval;
    int tb = 0, diff = 0;
    uint64_t mask = 0;
    U bits = 0;
    __syncthreads();  // the tables are there; the round before has read its zz
    if (live) {
      const int mx = (int)(i / lay.blocks_per_mcu), k = (int)(i - (long long)mx * lay.blocks_per_mcu);
      int c, brow, bcol, prow, pcol;  // the block, and the block before it of the same component in scan order
      if (k < luma_blocks) {
        c = 0;
        const int v = k / f.hs, u = k - v * f.hs;
        brow = my * f.vs + v; bcol = mx * f.hs + u;
        const int pk = k ? k - 1 : luma_blocks - 1, pv = pk / f.hs, pu = pk - pv * f.hs;
        prow = my * f.vs + pv; pcol = (k ? mx : mx - 1) * f.hs + pu;
      } else {
        c = k - luma_blocks + 1;
        brow = prow = my; bcol = mx; pcol = mx - 1;
      }
      tb = c ? 1 : 0;
      const int16_t *comp = coef + f.coef_off[c];
      const int16_t *blk = comp + ((long long)brow * f.block_cols[c] + bcol) * 64;
      const int pred = pcol < 0 ? 0 : comp[((long long)prow * f.block_cols[c] + pcol) * 64];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(blk + j * 8);
        const U rw[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int h = 0; h < 8; ++h) {
          int x = (int16_t)(h & 1 ? rw[h >> 1] >> 16 : rw[h >> 1] & 0xffffu);
          const int nat = j * 8 + h, pos = kZigzagOf.at[nat];
          if (nat == 0) {
            diff = x - pred;
            if (diff > 2047 || diff < -2047) { bad = true; diff = max(min(diff, 2047), -2047); }
            continue;
          }
          if (x > 1023 || x < -1023) { bad = true; x = max(min(x, 1023), -1023); }
          zz[pos * kHuffThreads + tid] = (int16_t)x;
          if (x) mask |= 1ull << pos;
        }
      }
      // the length
      bits = (dc_table[tb][bit_category(diff)] & 255u) + (U)bit_category(diff);
      int prev = 0;
      for (uint64_t m = mask; m; m &= m - 1) {
        const int pos = __ffsll((unsigned long long)m) - 1, run = pos - prev - 1, cat = bit_category(zz[pos * kHuffThreads + tid]);
        prev = pos;
        bits += (U)(run >> 4) * (ac_table[tb][0xF0] & 255u) + (ac_table[tb][((run & 15) << 4) | cat] & 255u) + (U)cat;
      }
      if (prev != 63) bits += ac_table[tb][0] & 255u;
    }
    U round_bits;
    const U at = base_bits + block_exclusive_scan(bits, wave_sums, &round_bits);
    // the words this round is the first to touch: those that begin at or after base_bits
    for (U wi = (base_bits + 31) / 32 + tid; wi < (base_bits + round_bits + 31) / 32; wi += kHuffThreads) slab[wi] = 0;
    __syncthreads();
    if (live) {
      BitWriter bw = {slab + at / 32, 0, (int)(at & 31)};
      int cat = bit_category(diff);
      U e = dc_table[tb][cat];
      bw.put(e >> 8, (int)(e & 255u));
      if (cat) bw.put((U)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1u), cat);
      int prev = 0;
      for (uint64_t m = mask; m; m &= m - 1) {
        const int pos = __ffsll((unsigned long long)m) - 1, x = zz[pos * kHuffThreads + tid];
        int run = pos - prev - 1;
        prev = pos;
        cat = bit_category(x);
        e = ac_table[tb][0xF0];
        for (; run > 15; run -= 16) bw.put(e >> 8, (int)(e & 255u));
        e = ac_table[tb][(run << 4) | cat];
        bw.put(((e >> 8) << cat) | ((U)(x < 0 ? x - 1 : x) & ((1u << cat) - 1u)), (int)(e & 255u) + cat);
      }
      if (prev != 63) {
        e = ac_table[tb][0];
        bw.put(e >> 8, (int)(e & 255u));
      }
      bw.finish();
    }
    base_bits += round_bits;
  }
  const bool any_bad = __syncthreads_or(bad);  // and every bit of the interval is in the slab (atomics, so in L2)
  // the stuffed length: the bytes, the last one padded with 1-bits, and one more for every FF among them
  const U nbytes = (base_bits + 7) / 8, rem = base_bits & 7;
  U ff = 0;
  for (U wi = tid; wi * 4 < nbytes; wi += kHuffThreads) {
    U w = __hip_atomic_load(slab + wi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const U at = wi * 4 + j;
      U byte = (w >> (24 - 8 * j)) & 0xffu;
      if (at == nbytes - 1 && rem) byte |= 0xffu >> rem;
      if (at < nbytes && byte == 0xffu) ++ff;
    }
  }
  U total_ff;
  block_exclusive_scan(ff, wave_sums, &total_ff);
  if (tid == 0) {
    record[0] = (nbytes + total_ff) | (any_bad ? kRecordBad : 0u);
    record[1] = base_bits;
  }
}

// grid (most MCU rows of a frame, n_frames), one workgroup an interval: where the interval begins in the stream (the stuffed
// lengths of the intervals before it, two bytes of marker each), then its bytes 1024 at a time -- a scan over the FF counts
// places every byte -- then RSTm, or EOI and the frame's result behind the last interval.  Nothing is stored at or past the
// frame's capacity.
__global__ __launch_bounds__(kHuffThreads) void jpeg_compact_kernel(const bfhip_jpeg_enc_frame *__restrict__ frames,
                                                                   const uint8_t *__restrict__ workspace, uint8_t *__restrict__ out,
                                                                   int64_t *__restrict__ result) {
  __shared__ U wave_sums[kHuffThreads / 64 + 1];
  __shared__ unsigned long long begin_sum;
  const bfhip_jpeg_enc_frame &f = frames[blockIdx.y];
  const EncLayout lay = enc_layout(f.width, f.height, f.hs, f.vs);
  const int my = blockIdx.x;
  if (my >= lay.mcus_y) return;
  const int tid = threadIdx.x;
  const uint8_t *ws = workspace + f.ws_off;
  const U *records = reinterpret_cast<const U *>(ws);
  const U *slab = reinterpret_cast<const U *>(ws + lay.slab_at + lay.slab_bytes_per_interval * (size_t)my);
  if (tid == 0) begin_sum = 0;
  __syncthreads();
  unsigned long long mine = 0;
  U bad = records[2 * my] & kRecordBad;
  for (int k = tid; k < my; k += kHuffThreads) {
    mine += (unsigned long long)(records[2 * k] & ~kRecordBad) + 2;
    bad |= records[2 * k] & kRecordBad;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d, 64);
  if ((tid & 63) == 0) atomicAdd(&begin_sum, mine);
  const bool any_bad = __syncthreads_or(bad != 0);
  const long long begin = (long long)begin_sum, cap = f.capacity;
  uint8_t *dst = out + f.out_off;
  const U stuffed = records[2 * my] & ~kRecordBad, bits = records[2 * my + 1], nbytes = (bits + 7) / 8, rem = bits & 7;
  U ff_before = 0;
  for (U first = 0; first * 4 < nbytes; first += kHuffThreads) {
    const U wi = first + tid;
    U byte[4], ff = 0;
    if (wi * 4 < nbytes) {
      const U w = slab[wi];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const U at = wi * 4 + j;
        byte[j] = (w >> (24 - 8 * j)) & 0xffu;
        if (at == nbytes - 1 && rem) byte[j] |= 0xffu >> rem;
        if (at < nbytes && byte[j] == 0xffu) ++ff;
      }
    }
    U round_ff;
    const U before = ff_before + block_exclusive_scan(ff, wave_sums, &round_ff);
    if (wi * 4 < nbytes) {
      long long p = begin + (long long)wi * 4 + before;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (wi * 4 + j >= nbytes) break;
        if (p < cap) dst[p] = (uint8_t)byte[j];
        ++p;
        if (byte[j] == 0xffu) {
          if (p < cap) dst[p] = 0;
          ++p;
        }
      }
    }
    ff_before += round_ff;
  }
  if (tid == 0) {
    const long long p = begin + stuffed;
    const bool last = my == lay.mcus_y - 1;
    if (p < cap) dst[p] = 0xFF;
    if (p + 1 < cap) dst[p + 1] = last ? 0xD9 : (uint8_t)(0xD0 + (my & 7));
    if (last) {
      result[2 * blockIdx.y] = p + 2;
      result[2 * blockIdx.y + 1] = (any_bad ? BFHIP_JPEG_ENC_BAD_COEF : 0) | (p + 2 > cap ? BFHIP_JPEG_ENC_OVERFLOW : 0);
    }
  }
}

static bool sampling_ok(int hs, int vs) { return (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2); }

// Validates the host copy of the table.  what: bit 0 the pixels, bit 1 the workspace and the output.
static int validate_frames(const char *who, const bfhip_jpeg_enc_frame *frames, int n_frames, int what, size_t rgb_bytes,
                           size_t coef_elems, size_t workspace_bytes, size_t out_bytes, long long *most_blocks, int *most_rows) {
  BFHIP_REQUIRE(n_frames >= 1 && n_frames <= 65535, "%s: n_frames=%d outside 1..65535", who, n_frames);
  long long out_end = 0, ws_end = 0;
  *most_blocks = 0;
  *most_rows = 0;
  for (int i = 0; i < n_frames; ++i) {
    const bfhip_jpeg_enc_frame &f = frames[i];
    BFHIP_REQUIRE(f.width >= 1 && f.height >= 1 && f.width <= 65535 && f.height <= 65535 && sampling_ok(f.hs, f.vs),
                  "%s: frame %d: %dx%d sampling %dx%d", who, i, f.width, f.height, f.hs, f.vs);
    const EncLayout lay = enc_layout(f.width, f.height, f.hs, f.vs);
    long long blocks = 0;
    for (int c = 0; c < 3; ++c) {
      BFHIP_REQUIRE(f.block_cols[c] == lay.mcus_x * (c ? 1 : f.hs) && f.block_rows[c] == lay.mcus_y * (c ? 1 : f.vs),
                    "%s: frame %d component %d: %d x %d blocks do not fit the frame", who, i, c, f.block_rows[c], f.block_cols[c]);
      const long long nb = (long long)f.block_cols[c] * f.block_rows[c];
      BFHIP_REQUIRE(f.coef_off[c] >= 0 && f.coef_off[c] % 8 == 0 && (unsigned long long)(f.coef_off[c] + nb * 64) <= coef_elems,
                    "%s: frame %d component %d: coefficients outside the buffer", who, i, c);
      for (int k = 0; k < 64; ++k)
        BFHIP_REQUIRE(f.quant[c][k] >= 1, "%s: frame %d component %d: quantisation entry %d is zero", who, i, c, k);
      blocks += nb;
    }
    if (what & 1)
      BFHIP_REQUIRE(f.rgb_off >= 0 && (unsigned long long)(f.rgb_off + (long long)f.width * f.height * 3) <= rgb_bytes,
                    "%s: frame %d: pixels outside the input block", who, i);
    if (what & 2) {
      BFHIP_REQUIRE(f.capacity >= 0 && f.out_off >= out_end && (unsigned long long)(f.out_off + f.capacity) <= out_bytes,
                    "%s: frame %d: its output overlaps the frame before or leaves the buffer", who, i);
      BFHIP_REQUIRE(f.ws_off >= ws_end && f.ws_off % 256 == 0 && (unsigned long long)f.ws_off + lay.total <= workspace_bytes,
                    "%s: frame %d: its workspace overlaps the frame before or leaves the buffer", who, i);
      out_end = f.out_off + f.capacity;
      ws_end = f.ws_off + (long long)lay.total;
    }
    *most_blocks = blocks > *most_blocks ? blocks : *most_blocks;
    *most_rows = lay.mcus_y > *most_rows ? lay.mcus_y : *most_rows;
  }
  return BFHIP_OK;
}

static int launch_forward(const bfhip_jpeg_enc_frame *frames_dev, int n_frames, long long most_blocks, const uint8_t *rgb_dev,
                          int16_t *coef_dev, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_forward_kernel, dim3((unsigned)ceil_div(most_blocks, kFwdBlocks), (unsigned)n_frames), dim3(kFwdThreads), 0,
                     s, frames_dev, rgb_dev, coef_dev);
  return check_launch("jpeg_forward_kernel");
}

static int launch_entropy(const bfhip_jpeg_enc_frame *frames_dev, int n_frames, int most_rows, const int16_t *coef_dev,
                          uint8_t *workspace, uint8_t *out_dev, int64_t *result_dev, hipStream_t s) {
  hipLaunchKernelGGL(jpeg_huffman_kernel, dim3((unsigned)most_rows, (unsigned)n_frames), dim3(kHuffThreads), 0, s, frames_dev,
                     coef_dev, workspace);
  int rc = check_launch("jpeg_huffman_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)most_rows, (unsigned)n_frames), dim3(kHuffThreads), 0, s, frames_dev,
                     workspace, out_dev, result_dev);
  return check_launch("jpeg_compact_kernel");
}

}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_jpeg_entropy_encode(const bfhip_jpeg_header *header, const int16_t *coef, size_t coef_bytes,
                                           int restart_interval, uint8_t *out, size_t capacity, bfhip_jpeg_enc_stats *stats) {
  char err[bfjpeg_enc::kErrLen];
  const int rc = bfjpeg_enc::entropy_encode(header, coef, coef_bytes, restart_interval, out, capacity, stats, err);
  if (rc) set_error("%s", err);
  return rc;
}

BFHIP_EXPORT int bfhip_jpeg_encode_supported(int width, int height, int hs, int vs) {
  return width >= 1 && height >= 1 && width <= 65535 && height <= 65535 && sampling_ok(hs, vs) ? 1 : 0;
}

BFHIP_EXPORT size_t bfhip_jpeg_encode_workspace_bytes(int width, int height, int hs, int vs) {
  if (!bfhip_jpeg_encode_supported(width, height, hs, vs)) return 0;
  return enc_layout(width, height, hs, vs).total;
}

BFHIP_EXPORT int bfhip_jpeg_encode_max_frames(void) { return 65535; }

#define BFHIP_JPEG_ENC_ALIGNED(who)                                                                                        \
  BFHIP_REQUIRE((reinterpret_cast<uintptr_t>(coef_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(frames_dev) & 15) == 0, \
                who ": coef_dev and frames_dev must be 16-byte aligned")

BFHIP_EXPORT int bfhip_jpeg_forward(const bfhip_jpeg_enc_frame *frames_host, const bfhip_jpeg_enc_frame *frames_dev, int n_frames,
                                    const uint8_t *rgb_dev, size_t rgb_bytes, int16_t *coef_dev, size_t coef_elems, void *stream) {
  BFHIP_REQUIRE(frames_host && frames_dev && rgb_dev && coef_dev, "bfhip_jpeg_forward: null argument");
  BFHIP_JPEG_ENC_ALIGNED("bfhip_jpeg_forward");
  long long most_blocks;
  int most_rows;
  const int rc = validate_frames("bfhip_jpeg_forward", frames_host, n_frames, 1, rgb_bytes, coef_elems, 0, 0, &most_blocks, &most_rows);
  if (rc) return rc;
  return launch_forward(frames_dev, n_frames, most_blocks, rgb_dev, coef_dev, (hipStream_t)stream);
}

BFHIP_EXPORT int bfhip_jpeg_entropy_encode_device(const bfhip_jpeg_enc_frame *frames_host, const bfhip_jpeg_enc_frame *frames_dev,
                                                  int n_frames, const int16_t *coef_dev, size_t coef_elems, void *workspace,
                                                  size_t workspace_bytes, uint8_t *out_dev, size_t out_bytes, int64_t *result_dev,
                                                  void *stream) {
  BFHIP_REQUIRE(frames_host && frames_dev && coef_dev && workspace && out_dev && result_dev,
                "bfhip_jpeg_entropy_encode_device: null argument");
  BFHIP_JPEG_ENC_ALIGNED("bfhip_jpeg_entropy_encode_device");
  BFHIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(result_dev) & 7) == 0,
                "bfhip_jpeg_entropy_encode_device: the workspace must be 256-byte and result_dev 8-byte aligned");
  long long most_blocks;
  int most_rows;
  int rc = validate_frames("bfhip_jpeg_entropy_encode_device", frames_host, n_frames, 2, 0, coef_elems, workspace_bytes, out_bytes,
                           &most_blocks, &most_rows);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  return launch_entropy(frames_dev, n_frames, most_rows, coef_dev, (uint8_t *)workspace, out_dev, result_dev, s);
}

BFHIP_EXPORT int bfhip_jpeg_encode(const bfhip_jpeg_enc_frame *frames_host, const bfhip_jpeg_enc_frame *frames_dev, int n_frames,
                                   const uint8_t *rgb_dev, size_t rgb_bytes, int16_t *coef_dev, size_t coef_elems, void *workspace,
                                   size_t workspace_bytes, uint8_t *out_dev, size_t out_bytes, int64_t *result_dev, void *stream) {
  BFHIP_REQUIRE(frames_host && frames_dev && rgb_dev && coef_dev && workspace && out_dev && result_dev, "bfhip_jpeg_encode: null argument");
  BFHIP_JPEG_ENC_ALIGNED("bfhip_jpeg_encode");
  BFHIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 && (reinterpret_cast<uintptr_t>(result_dev) & 7) == 0,
                "bfhip_jpeg_encode: the workspace must be 256-byte and result_dev 8-byte aligned");
  long long most_blocks;
  int most_rows;
  int rc = validate_frames("bfhip_jpeg_encode", frames_host, n_frames, 3, rgb_bytes, coef_elems, workspace_bytes, out_bytes,
                           &most_blocks, &most_rows);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = launch_forward(frames_dev, n_frames, most_blocks, rgb_dev, coef_dev, s);
  if (rc) return rc;
  return launch_entropy(frames_dev, n_frames, most_rows, coef_dev, (uint8_t *)workspace, out_dev, result_dev, s);
}
