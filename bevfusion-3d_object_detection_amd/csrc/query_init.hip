// query_init.hip -- query initialisation of the TransFusion head (BF/bevfusion_head.py:221-260,278-281): 3x3 peak test on the
// score map, the K best of the C*H*W masked scores in a DEFINED order, and the gather of everything the head reads at the picks.
//
// Order: (masked score descending, flat index c*HW + y*W + x ascending).  A positive peak becomes the 64-bit key
//   (score bits << 32) | ~flat: positive floats order like their bit patterns, the inverted index breaks ties towards the lower
//   index, and every key is unique, so "the K largest keys" is one fixed set in one fixed order whatever the append order was.
//
// Launches: memset of the counters, qi_peak_kernel over the map (one counter add per workgroup), qi_select_kernel with one workgroup per sample (threshold,
//   sort, zero fill, and all five outputs).  Backward: memset of d_flat + qi_bwd_kernel, one workgroup per sample.
// Only integer atomics are used (candidate count, histograms); no float is ever added out of order.
#include "common.h"

namespace bfhip {
namespace {

constexpr int kBins = 2048;        // histogram over key >> 52: sign (0), 8 exponent and 3 mantissa bits of the score
constexpr int kBinShift = 52;
constexpr int kMaxK = 512;         // picks per sample one workgroup sorts and resolves
constexpr int kSelThreads = 1024;  // select / backward workgroup; also the size of the LDS sort
constexpr int kPeakThreads = 256;
constexpr int kPeakItems = 8;      // cells per thread of the peak pass
constexpr int kBatch = 8;          // candidate keys a thread of the select pass loads before it looks at any

typedef unsigned long long u64;

struct Map {  // the score map with its strides in elements; `cl`: the class axis is the fastest in memory
  const float *h;
  long long sb, sc, sy, sx;
  int C, H, W, cl;
  unsigned nms_free;  // bit c: class c skips the window test
};

// m of one cell: the score where it is a positive 3x3 peak of its class plane (or its class is NMS-free), else 0.
// NaN, zero and negative scores give 0; a NaN neighbour fails the comparison, as torch's max_pool2d would make it.
__device__ __forceinline__ float masked_score(const Map &m, int b, int c, int y, int x) {
  const float *p = m.h + b * m.sb + c * m.sc + y * m.sy + x * m.sx;
  const float v = *p;
  if (!(v > 0.f)) return 0.f;
  if ((m.nms_free >> c) & 1u) return v;
  if (y < 1 || y > m.H - 2 || x < 1 || x > m.W - 2) return 0.f;
  bool ok = true;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
      if (dy != 0 || dx != 0) ok &= (v >= p[dy * m.sy + dx * m.sx]);
  return ok ? v : 0.f;
}

__device__ __forceinline__ unsigned lanes_below(u64 mask, int lane) { return (unsigned)__popcll(mask & ((1ull << lane) - 1ull)); }

// ---- pass 1: positive peaks -> candidate keys + per-sample histogram of their top bits
// A workgroup ranks its peaks in LDS and reserves their slots with ONE integer atomic (thousands of adds to the one counter of
// a sample serialise at the memory side); the histogram is privatised in LDS and flushed once.
__global__ __launch_bounds__(kPeakThreads) void qi_peak_kernel(Map m, unsigned N, unsigned *count, unsigned *hist, u64 *cand) {
  __shared__ unsigned sh[kBins];
  __shared__ unsigned s_wave[kPeakThreads / 64];
  __shared__ unsigned s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  for (int i = tid; i < kBins; i += kPeakThreads) sh[i] = 0;
  __syncthreads();
  const unsigned HW = (unsigned)(m.H * m.W);
  const unsigned base = blockIdx.x * (unsigned)(kPeakThreads * kPeakItems);
  float v[kPeakItems];
  unsigned f[kPeakItems];
  unsigned in_wave = 0;  // peaks of this wave (wave-uniform)
#pragma unroll
  for (int it = 0; it < kPeakItems; ++it) {
    const unsigned t = base + it * kPeakThreads + tid;  // walks the map in its memory order
    v[it] = 0.f;
    f[it] = 0;
    if (t < N) {
      unsigned c, cell;
      if (m.cl) { c = t % (unsigned)m.C; cell = t / (unsigned)m.C; }
      else { c = t / HW; cell = t % HW; }
      f[it] = c * HW + cell;
      v[it] = masked_score(m, b, (int)c, (int)(cell / (unsigned)m.W), (int)(cell % (unsigned)m.W));
    }
    in_wave += (unsigned)__popcll(__ballot(v[it] > 0.f));
  }
  if (lane == 0) s_wave[wave] = in_wave;
  __syncthreads();
  if (tid == 0) {
    unsigned total = 0;
    for (int w = 0; w < kPeakThreads / 64; ++w) total += s_wave[w];
    s_base = total ? atomicAdd(&count[b], total) : 0u;
  }
  __syncthreads();
  unsigned slot = s_base;
  for (int w = 0; w < wave; ++w) slot += s_wave[w];
#pragma unroll
  for (int it = 0; it < kPeakItems; ++it) {
    const bool is = v[it] > 0.f;
    const u64 mask = __ballot(is);
    if (is) {
      const u64 key = ((u64)__float_as_uint(v[it]) << 32) | (u64)(unsigned)~f[it];
      const unsigned at = slot + lanes_below(mask, lane);
      if (at < N) cand[(size_t)b * N + at] = key;
      atomicAdd(&sh[(unsigned)(key >> kBinShift)], 1u);
    }
    slot += (unsigned)__popcll(mask);
  }
  __syncthreads();
  for (int i = tid; i < kBins; i += kPeakThreads)
    if (sh[i]) atomicAdd(&hist[(size_t)b * kBins + i], sh[i]);
}

struct Out {
  long long *top_class, *top_index;
  float *pos, *score;
  void *rows;
  const void *flat;        // rows of the BEV features: element (b, cell, ch) at b * fb + cell * fr + ch
  long long fb, fr;
  int Ch, esize, K, pos_w;
};

// ---- pass 2: one workgroup per sample: threshold from the histogram, refinement over the candidates while the boundary bin is
// too full, LDS sort of the survivors, zero fill, outputs
__global__ __launch_bounds__(kSelThreads) void qi_select_kernel(Map m, unsigned N, const unsigned *count, const unsigned *hist,
                                                                const u64 *cand, Out o) {
  __shared__ u64 keys[kSelThreads];
  __shared__ unsigned scan[2][kSelThreads];
  __shared__ unsigned dh[256];
  __shared__ unsigned sidx[kMaxK];
  __shared__ unsigned wt[kSelThreads / 64];
  __shared__ u64 s_prefix;
  __shared__ unsigned s_need, s_inbin, s_cnt;
  __shared__ int s_lo;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const unsigned K = (unsigned)o.K;
  const unsigned HW = (unsigned)(m.H * m.W);
  unsigned n = count[b];
  if (n > N) n = N;
  const u64 *cb = cand + (size_t)b * N;
  const bool take_all = n <= (unsigned)kSelThreads;  // everything fits the sort (covers "fewer than K positive peaks")

  if (tid == 0) { s_cnt = 0; s_lo = 0; s_prefix = 0; s_need = 0; s_inbin = 0; }
  __syncthreads();
  if (!take_all) {
    // bin t with count(bins > t) < K <= count(bins >= t): inclusive suffix sums over the 2048 bins, two per thread
    const unsigned *hb = hist + (size_t)b * kBins;
    const unsigned h0 = hb[2 * tid], h1 = hb[2 * tid + 1];
    scan[0][tid] = h0 + h1;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kSelThreads; off <<= 1) {
      const unsigned v = scan[cur][tid] + (tid + off < kSelThreads ? scan[cur][tid + off] : 0u);
      scan[cur ^ 1][tid] = v;
      __syncthreads();
      cur ^= 1;
    }
    const unsigned incl0 = scan[cur][tid];  // candidates in bins >= 2 tid
    const unsigned incl1 = incl0 - h0;      // candidates in bins >= 2 tid + 1
    const unsigned above1 = incl1 - h1;
    if (incl1 >= K && above1 < K) { s_prefix = 2 * tid + 1; s_need = K - above1; s_inbin = h1; s_lo = kBinShift; }
    if (incl0 >= K && incl1 < K) { s_prefix = 2 * tid; s_need = K - incl1; s_inbin = h0; s_lo = kBinShift; }
    __syncthreads();
    // radix refinement, 8 key bits a pass: rare (a plateau of equal scores, or a crowded bin)
    while (true) {
      const unsigned inbin = s_inbin;
      const int lo = s_lo;
      const u64 prefix = s_prefix;
      if (inbin <= (unsigned)kMaxK || lo == 0) break;
      const int d = lo < 8 ? lo : 8, nlo = lo - d;
      if (tid < 256) dh[tid] = 0;
      __syncthreads();
      for (unsigned i0 = tid; i0 < n; i0 += kSelThreads * kBatch) {
        u64 k[kBatch];  // the loads of a batch are in flight together (0 is no key: a key has a positive score)
#pragma unroll
        for (int j = 0; j < kBatch; ++j) k[j] = i0 + j * kSelThreads < n ? cb[i0 + j * kSelThreads] : 0ull;
#pragma unroll
        for (int j = 0; j < kBatch; ++j)
          if (k[j] != 0 && (k[j] >> lo) == prefix) atomicAdd(&dh[(unsigned)(k[j] >> nlo) & ((1u << d) - 1u)], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        const unsigned need = s_need;
        unsigned cum = 0;
        int g = (1 << d) - 1;
        for (; g > 0; --g) {
          if (cum + dh[g] >= need) break;
          cum += dh[g];
        }
        s_need = need - cum;
        s_inbin = dh[g];
        s_prefix = (prefix << d) | (u64)g;
        s_lo = nlo;
      }
      __syncthreads();
    }
  }
  {
    // survivors: keys above the boundary prefix (fewer than K) and the boundary group (at most kMaxK) -> at most 1023
    const int lo = s_lo;
    const u64 prefix = s_prefix;
    for (unsigned i0 = tid; i0 < n; i0 += kSelThreads * kBatch) {
      u64 k[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) k[j] = i0 + j * kSelThreads < n ? cb[i0 + j * kSelThreads] : 0ull;
#pragma unroll
      for (int j = 0; j < kBatch; ++j)
        if (k[j] != 0 && (take_all || (k[j] >> lo) >= prefix)) {
          const unsigned pos = atomicAdd(&s_cnt, 1u);
          if (pos < (unsigned)kSelThreads) keys[pos] = k[j];
        }
    }
  }
  __syncthreads();
  unsigned cnt = s_cnt;
  if (cnt > (unsigned)kSelThreads) cnt = kSelThreads;
  if ((unsigned)tid >= cnt) keys[tid] = 0;  // below every real key (a real key has a positive score)
  __syncthreads();
  for (int k = 2; k <= kSelThreads; k <<= 1) {  // bitonic sort, descending
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int other = tid ^ j;
      if (other > tid) {
        const u64 a = keys[tid], c = keys[other];
        const bool desc = (tid & k) == 0;
        if (desc ? a < c : a > c) { keys[tid] = c; keys[other] = a; }
      }
      __syncthreads();
    }
  }
  const unsigned npos = cnt < K ? cnt : K;
  if ((unsigned)tid < npos) sidx[tid] = ~(unsigned)keys[tid];
  // fewer than K positive peaks: the zero-valued cells in ascending flat index, then (only when those run out) the NaN cells
  unsigned filled = npos;
  for (int phase = 0; phase < 2 && filled < K; ++phase) {
    for (unsigned base = 0; base < N && filled < K; base += kSelThreads) {
      const unsigned f = base + tid;
      bool pick = false;
      if (f < N) {
        const int c = (int)(f / HW), y = (int)((f % HW) / (unsigned)m.W), x = (int)((f % HW) % (unsigned)m.W);
        const float v = m.h[b * m.sb + c * m.sc + y * m.sy + x * m.sx];
        const bool nan = v != v;
        pick = phase == 0 ? (!nan && !(masked_score(m, b, c, y, x) > 0.f)) : nan;
      }
      const u64 mask = __ballot(pick);
      if (lane == 0) wt[wave] = (unsigned)__popcll(mask);
      __syncthreads();
      unsigned before = 0, total = 0;
      for (int w = 0; w < kSelThreads / 64; ++w) {
        if (w < wave) before += wt[w];
        total += wt[w];
      }
      const unsigned pos = filled + before + lanes_below(mask, lane);
      if (pick && pos < K) sidx[pos] = f;
      filled = filled + total < K ? filled + total : K;
      __syncthreads();
    }
  }
  __syncthreads();

  // ---- outputs
  for (unsigned p = tid; p < K; p += kSelThreads) {
    const unsigned f = sidx[p], cell = f % HW;
    const size_t at = (size_t)b * K + p;
    o.top_class[at] = (long long)(f / HW);
    o.top_index[at] = (long long)cell;
    o.pos[at * 2 + 0] = (float)(cell / (unsigned)o.pos_w) + 0.5f;
    o.pos[at * 2 + 1] = (float)(cell % (unsigned)o.pos_w) + 0.5f;
  }
  for (unsigned u = tid; u < (unsigned)m.C * K; u += kSelThreads) {  // m of every class at the picked cell
    const unsigned c = u / K, p = u % K, cell = sidx[p] % HW;
    o.score[((size_t)b * m.C + c) * K + p] = masked_score(m, b, (int)c, (int)(cell / (unsigned)m.W), (int)(cell % (unsigned)m.W));
  }
  const unsigned vpr = (unsigned)(o.Ch * o.esize) / 16u;  // 16-byte vectors per row
  for (unsigned u = tid; u < K * vpr; u += kSelThreads) {
    const unsigned p = u / vpr, v = u % vpr, cell = sidx[p] % HW;
    const uint4 *src = (const uint4 *)((const char *)o.flat + ((size_t)b * o.fb + (size_t)cell * o.fr) * o.esize) + v;
    uint4 *dst = (uint4 *)((char *)o.rows + ((size_t)b * K + p) * (size_t)o.Ch * o.esize) + v;
    *dst = *src;
  }
}

// ---- backward of the row gather: the lowest pick of a cell sums its duplicates in ascending pick order, fp32, one rounding
template <bool BF>
__global__ __launch_bounds__(kSelThreads) void qi_bwd_kernel(const long long *top_index, const void *drows, void *dflat, int K, int Ch,
                                                             long long HW) {
  constexpr int VEC = BF ? 8 : 4;  // elements per 16-byte vector
  __shared__ int idx[kMaxK];
  __shared__ int nxt[kMaxK];
  __shared__ int own[kMaxK];
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int p = tid; p < K; p += kSelThreads) {
    const long long i = top_index[(size_t)b * K + p];
    idx[p] = (i >= 0 && i < HW) ? (int)i : -1;
  }
  __syncthreads();
  for (int p = tid; p < K; p += kSelThreads) {
    const int me = idx[p];
    int first = me >= 0, nx = K;
    for (int q = 0; q < K; ++q) {  // no early exit: independent broadcast reads, pipelined
      const bool eq = idx[q] == me;
      if (eq && q < p) first = 0;
      if (eq && q > p && q < nx) nx = q;
    }
    own[p] = first;
    nxt[p] = nx < K ? nx : -1;
  }
  __syncthreads();
  const int vpr = Ch / VEC;
  for (int u = tid; u < K * vpr; u += kSelThreads) {
    const int p = u / vpr, v = u % vpr;
    if (!own[p]) continue;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    bool head = true;
    for (int q = p; q >= 0; q = nxt[q]) {
      const uint4 w = *((const uint4 *)((const char *)drows + ((size_t)b * K + q) * (size_t)Ch * (BF ? 2 : 4)) + v);
      const unsigned ws[4] = {w.x, w.y, w.z, w.w};
      float g[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        g[e] = BF ? __uint_as_float((e & 1) ? (ws[e >> 1] & 0xffff0000u) : (ws[e >> 1] << 16)) : __uint_as_float(ws[e & 3]);
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = head ? g[e] : acc[e] + g[e];
      head = false;
    }
    uint4 r;
    if (BF) {
      unsigned pk[4];
#pragma unroll
      // every NaN becomes 0x7fc0: the CPU cases compare this gradient against torch's own conversion
      for (int e = 0; e < 4; ++e) pk[e] = bf16_rne_nan_canonical(acc[2 * e]) | (bf16_rne_nan_canonical(acc[2 * e + 1]) << 16);
      r = make_uint4(pk[0], pk[1], pk[2], pk[3]);
    } else {
      r = make_uint4(__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]), __float_as_uint(acc[3]));
    }
    *((uint4 *)((char *)dflat + ((size_t)b * HW + idx[p]) * (size_t)Ch * (BF ? 2 : 4)) + v) = r;
  }
}

bool shape_ok(int B, int C, int H, int W, int K, int Ch, int nms_kernel_size, int row_dtype) {
  if (B < 1 || B > 65535 || C < 1 || C > 32 || H < 3 || W < 3 || K < 1 || K > kMaxK || Ch < 1) return false;
  if (nms_kernel_size != 3 || (row_dtype != 0 && row_dtype != 1)) return false;
  const long long N = (long long)C * H * W;
  if (N >= (1ll << 31) || K > N) return false;
  return (Ch * (row_dtype ? 2 : 4)) % 16 == 0;
}

size_t header_bytes(int B) { return align_up((size_t)B * (1 + kBins) * sizeof(unsigned), 256); }

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_query_init_supported(int B, int C, int H, int W, int K, int Ch, int nms_kernel_size, int row_dtype) {
  return shape_ok(B, C, H, W, K, Ch, nms_kernel_size, row_dtype) ? 1 : 0;
}

BFHIP_EXPORT size_t bfhip_query_init_workspace_bytes(int B, int C, int H, int W) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
  return header_bytes(B) + (size_t)B * C * H * W * sizeof(u64);
}

BFHIP_EXPORT int bfhip_query_init_fwd(const float *h, long long h_sb, long long h_sc, long long h_sy, long long h_sx, int B, int C,
                                      int H, int W, unsigned nms_free_mask, const void *flat, long long flat_sb, long long flat_sr,
                                      int Ch, int row_dtype, int K, int pos_w, long long *top_class, long long *top_index,
                                      float *query_pos, float *query_heatmap_score, void *rows, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  BFHIP_REQUIRE(shape_ok(B, C, H, W, K, Ch, 3, row_dtype), "query_init_fwd: unsupported shape B=%d C=%d H=%d W=%d K=%d Ch=%d dtype=%d",
                B, C, H, W, K, Ch, row_dtype);
  BFHIP_REQUIRE(h && flat && top_class && top_index && query_pos && query_heatmap_score && rows && workspace, "query_init_fwd: null pointer");
  BFHIP_REQUIRE(pos_w >= 1, "query_init_fwd: pos_w %d", pos_w);
  BFHIP_REQUIRE(h_sb >= 0 && h_sc >= 1 && h_sy >= 1 && h_sx >= 1, "query_init_fwd: score map strides must be positive");
  const int esize = row_dtype ? 2 : 4;
  BFHIP_REQUIRE(flat_sr >= Ch && flat_sb >= 0 && (flat_sr * esize) % 16 == 0 && (flat_sb * esize) % 16 == 0 &&
                    ((uintptr_t)flat % 16) == 0 && ((uintptr_t)rows % 16) == 0,
                "query_init_fwd: feature rows must be 16-byte aligned");
  BFHIP_REQUIRE(workspace_bytes >= bfhip_query_init_workspace_bytes(B, C, H, W) && ((uintptr_t)workspace % 16) == 0,
                "query_init_fwd: workspace too small or unaligned");
  hipStream_t s = (hipStream_t)stream;
  const unsigned N = (unsigned)((long long)C * H * W);
  unsigned *count = (unsigned *)workspace;
  unsigned *hist = count + B;
  u64 *cand = (u64 *)((char *)workspace + header_bytes(B));
  if (hipMemsetAsync(workspace, 0, header_bytes(B), s) != hipSuccess) return check_launch("query_init_fwd memset");
  Map m{h, h_sb, h_sc, h_sy, h_sx, C, H, W, (h_sc == 1 && C > 1) ? 1 : 0, nms_free_mask};
  dim3 grid(ceil_div(N, kPeakThreads * kPeakItems), B);
  hipLaunchKernelGGL(qi_peak_kernel, grid, dim3(kPeakThreads), 0, s, m, N, count, hist, cand);
  int rc = check_launch("qi_peak_kernel");
  if (rc) return rc;
  Out o{top_class, top_index, query_pos, query_heatmap_score, rows, flat, flat_sb, flat_sr, Ch, esize, K, pos_w};
  hipLaunchKernelGGL(qi_select_kernel, dim3(B), dim3(kSelThreads), 0, s, m, N, (const unsigned *)count, (const unsigned *)hist,
                     (const u64 *)cand, o);
  return check_launch("qi_select_kernel");
}

BFHIP_EXPORT int bfhip_query_init_bwd(const long long *top_index, const void *d_rows, int B, int K, int Ch, long long HW,
                                      int row_dtype, void *d_flat, void *stream) {
  BFHIP_REQUIRE(B >= 1 && B <= 65535 && K >= 1 && K <= kMaxK && HW >= 1 && (row_dtype == 0 || row_dtype == 1),
                "query_init_bwd: bad shape B=%d K=%d HW=%lld dtype=%d", B, K, HW, row_dtype);
  const int esize = row_dtype ? 2 : 4;
  BFHIP_REQUIRE(Ch >= 1 && (Ch * esize) % 16 == 0, "query_init_bwd: Ch=%d is not a whole number of 16-byte vectors", Ch);
  BFHIP_REQUIRE(top_index && d_rows && d_flat && ((uintptr_t)d_rows % 16) == 0 && ((uintptr_t)d_flat % 16) == 0,
                "query_init_bwd: null or unaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(d_flat, 0, (size_t)B * HW * Ch * esize, s) != hipSuccess) return check_launch("query_init_bwd memset");
  if (row_dtype)
    hipLaunchKernelGGL(qi_bwd_kernel<true>, dim3(B), dim3(kSelThreads), 0, s, top_index, d_rows, d_flat, K, Ch, HW);
  else
    hipLaunchKernelGGL(qi_bwd_kernel<false>, dim3(B), dim3(kSelThreads), 0, s, top_index, d_rows, d_flat, K, Ch, HW);
  return check_launch("qi_bwd_kernel");
}
