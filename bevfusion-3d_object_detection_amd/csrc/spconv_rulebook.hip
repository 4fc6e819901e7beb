// spconv_rulebook.hip -- rulebooks of the sparse convolutions (see spconv.hip for the layout conventions): the SubM hash
// builder, the strided bitmap + scan builder, the row masks with the chunked row sort, and the debug validator.
// The only unit that includes rocPRIM.
#include "spconv_common.h"

#include <rocprim/block/block_radix_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>

namespace bfhip {
namespace {

struct ConvGeom {
  int B;
  int in0, in1, in2;     // input spatial shape (X, Y, Z)
  int out0, out1, out2;  // output spatial shape
  int k0, k1, k2, s0, s1, s2, p0, p1, p2, d0, d1, d2;
  int KV;
};

inline unsigned table_cap(int n) {
  unsigned cap = 1024;
  while (cap < 2u * (unsigned)n) cap <<= 1;
  return cap;
}

inline int make_geom(int B, const int *in_shape, const int *ksize, const int *stride,
                     const int *padding, const int *dilation, bool subm, ConvGeom &G) {
  G.B = B;
  G.in0 = in_shape[0]; G.in1 = in_shape[1]; G.in2 = in_shape[2];
  G.k0 = ksize[0]; G.k1 = ksize[1]; G.k2 = ksize[2];
  G.d0 = dilation[0]; G.d1 = dilation[1]; G.d2 = dilation[2];
  if (subm) {
    G.s0 = G.s1 = G.s2 = 1;
    G.p0 = G.d0 * (G.k0 / 2); G.p1 = G.d1 * (G.k1 / 2); G.p2 = G.d2 * (G.k2 / 2);
    G.out0 = G.in0; G.out1 = G.in1; G.out2 = G.in2;
  } else {
    G.s0 = stride[0]; G.s1 = stride[1]; G.s2 = stride[2];
    G.p0 = padding[0]; G.p1 = padding[1]; G.p2 = padding[2];
    // (in + 2p - d(k-1) - 1)//s + 1   (projects/SparseConvolution/sparse_conv.py:88-90)
    G.out0 = (G.in0 + 2 * G.p0 - G.d0 * (G.k0 - 1) - 1) / G.s0 + 1;
    G.out1 = (G.in1 + 2 * G.p1 - G.d1 * (G.k1 - 1) - 1) / G.s1 + 1;
    G.out2 = (G.in2 + 2 * G.p2 - G.d2 * (G.k2 - 1) - 1) / G.s2 + 1;
  }
  G.KV = G.k0 * G.k1 * G.k2;
  if (B <= 0 || G.in0 <= 0 || G.in1 <= 0 || G.in2 <= 0 || G.KV <= 0 || G.KV > 64) return -1;
  if (G.s0 <= 0 || G.s1 <= 0 || G.s2 <= 0 || G.out0 <= 0 || G.out1 <= 0 || G.out2 <= 0) return -1;
  if ((long long)B * G.in0 * G.in1 * G.in2 >= 0x7fffffffLL) return -1;
  return 0;
}

__device__ __forceinline__ unsigned hash32(unsigned k) {
  k ^= k >> 16; k *= 0x85ebca6bu; k ^= k >> 13; k *= 0xc2b2ae35u; k ^= k >> 16;
  return k;
}

__global__ __launch_bounds__(256) void fill_pair_kernel(int2 *__restrict__ t, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) t[i] = make_int2(-1, 0x7f7f7f7f);
}

// ------------------------------------------------------------------------------- SubM rulebook
// hash table of (key, row) pairs interleaved in one int2 (one cache line per probe)
__global__ __launch_bounds__(256) void subm_insert_kernel(const int4 *__restrict__ indices, int N,
                                                          ConvGeom G, int2 *__restrict__ table,
                                                          unsigned mask) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  int4 c = indices[n];
  if (c.x < 0) return;  // inactive row of a capacity-sized tensor (spconv.py, static capacity mode)
  int key = ((c.x * G.in0 + c.y) * G.in1 + c.z) * G.in2 + c.w;
  unsigned s = hash32((unsigned)key) & mask;
  for (unsigned probe = 0; probe <= mask; ++probe) {
    int old = atomicCAS(&table[s].x, -1, key);
    if (old == -1 || old == key) break;
    s = (s + 1) & mask;
  }
  atomicMin(&table[s].y, n);  // duplicate coordinates (malformed input): lowest row wins, deterministically
}

// blockIdx.y = kernel offset k in the LOWER half (k <= KV/2).  A submanifold rulebook is symmetric:
// pair[k][n] = j  <=>  pair[KV-1-k][j] = n, so each found neighbour fills two entries and only half of the
// offsets are probed; the centre offset maps every row to itself.  pair_fwd must be pre-filled with -1.
__global__ __launch_bounds__(256) void subm_pairs_kernel(const int4 *__restrict__ indices, int N,
                                                         ConvGeom G, const int2 *__restrict__ table,
                                                         unsigned mask, int *__restrict__ pair_fwd,
                                                         int *__restrict__ n_pairs, int symmetric) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  int found = -1;
  if (n < N && indices[n].x >= 0) {
    int4 c = indices[n];
    int l = k % G.k2, j = (k / G.k2) % G.k1, i = k / (G.k2 * G.k1);
    int dx_ = (i - G.k0 / 2) * G.d0, dy_ = (j - G.k1 / 2) * G.d1, dz_ = (l - G.k2 / 2) * G.d2;
    if (dx_ == 0 && dy_ == 0 && dz_ == 0) {
      found = n;
    } else {
      int x = c.y + dx_, y = c.z + dy_, z = c.w + dz_;
      if (x >= 0 && x < G.in0 && y >= 0 && y < G.in1 && z >= 0 && z < G.in2) {
        int key = ((c.x * G.in0 + x) * G.in1 + y) * G.in2 + z;
        unsigned s = hash32((unsigned)key) & mask;
        for (unsigned probe = 0; probe <= mask; ++probe) {
          int2 e = table[s];
          if (e.x == key) { found = e.y; break; }
          if (e.x == -1) break;
          s = (s + 1) & mask;
        }
      }
    }
    if (found >= 0) {
      pair_fwd[(size_t)k * N + n] = found;
      if (symmetric && k != G.KV - 1 - k) pair_fwd[(size_t)(G.KV - 1 - k) * N + found] = n;
    }
  }
  // pair statistics: spread over 64 counters (one hot word saturates at ~88 atomics/us); summed by the host wrapper
  unsigned long long bal = __ballot(found >= 0);
  if (n_pairs && (threadIdx.x & 63) == 0 && bal) {
    int add = __popcll(bal) * ((symmetric && k != G.KV - 1 - k) ? 2 : 1);
    atomicAdd(&n_pairs[(blockIdx.x * 4 + (threadIdx.x >> 6) + k) & 63], add);
  }
}

// Row-block form of the SubM rulebook: a workgroup is 64 rows x (k0*k1) offset columns, each thread probes the k2 offsets of
// its (i, j) column for its row.  Every pair_fwd entry is written exactly once (holes included: no pre-fill of the table),
// the k-th plane's 64 entries of a wave are one coalesced store, and the row's offset mask is assembled in LDS, so the row
// mask, the identity permutation and the (region, mask) sort key leave in the same launch (what row_mask_kernel did in a
// second pass over the table).  No atomics on global memory: the pair count is the popcount of the masks.
template <int K2>
__global__ __launch_bounds__(1024) void subm_pairs_rows_kernel(const int4 *__restrict__ indices, int N, ConvGeom G,
                                                               const int2 *__restrict__ table, unsigned tmask,
                                                               int *__restrict__ pair_fwd, unsigned *__restrict__ row_mask,
                                                               unsigned *__restrict__ iota, unsigned *__restrict__ keys,
                                                               int regions, int *__restrict__ n_pairs) {
  __shared__ unsigned smask[64];
  const int lane = threadIdx.x, ty = threadIdx.y;
  const int n = blockIdx.x * 64 + lane;
  if (ty == 0) smask[lane] = 0u;
  __syncthreads();
  const int k2 = K2 ? K2 : G.k2;
  const int i = ty / G.k1, j = ty - i * G.k1;
  int4 c = n < N ? indices[n] : make_int4(-1, 0, 0, 0);
  const int x = c.y + (i - G.k0 / 2) * G.d0, y = c.z + (j - G.k1 / 2) * G.d1;
  const bool xy_ok = c.x >= 0 && x >= 0 && x < G.in0 && y >= 0 && y < G.in1;
  const bool centre_col = x == c.y && y == c.z;
  const int base = ((c.x * G.in0 + x) * G.in1 + y) * G.in2;
  unsigned bits = 0u;
  for (int l = 0; l < k2; ++l) {
    const int k = ty * k2 + l;
    const int z = c.w + (l - k2 / 2) * G.d2;
    int found = -1;
    if (xy_ok && z >= 0 && z < G.in2) {
      if (centre_col && z == c.w) {
        found = n;
      } else {
        const int key = base + z;
        unsigned s = hash32((unsigned)key) & tmask;
        for (unsigned probe = 0; probe <= tmask; ++probe) {
          int2 e = table[s];
          if (e.x == key) { found = e.y; break; }
          if (e.x == -1) break;
          s = (s + 1) & tmask;
        }
      }
    }
    if (n < N) pair_fwd[(size_t)k * N + n] = found;
    bits |= (found >= 0 ? 1u : 0u) << (k & 31);
  }
  if (bits) atomicOr(&smask[lane], bits);
  __syncthreads();
  if (ty == 0) {
    const unsigned m = smask[lane];
    if (n < N) {
      if (row_mask) row_mask[n] = m;
      if (iota) iota[n] = (unsigned)n;
      if (keys) keys[n] = (regions > 1 ? (unsigned)(((long long)n * regions) / N) << G.KV : 0u) | m;
    }
    if (n_pairs) {
      int cnt = __popc(m);
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
      if (lane == 0 && cnt) atomicAdd(&n_pairs[blockIdx.x & 63], cnt);
    }
  }
}

// ---------------------------------------------------------------------------- strided rulebook
__device__ __forceinline__ bool out_coord(const ConvGeom &G, int4 c, int k, int &ox, int &oy, int &oz) {
  int l = k % G.k2, j = (k / G.k2) % G.k1, i = k / (G.k2 * G.k1);
  ox = c.y + G.p0 - i * G.d0;
  oy = c.z + G.p1 - j * G.d1;
  oz = c.w + G.p2 - l * G.d2;
  if (ox < 0 || oy < 0 || oz < 0) return false;
  if (ox % G.s0 || oy % G.s1 || oz % G.s2) return false;
  ox /= G.s0; oy /= G.s1; oz /= G.s2;
  return ox < G.out0 && oy < G.out1 && oz < G.out2;
}

// n_dev (optional): the true number of input rows lives on the device (N is then the host-side bound of the launch)
__global__ __launch_bounds__(256) void sparse_mark_kernel(const int4 *__restrict__ indices, int N,
                                                          const int *__restrict__ n_dev, ConvGeom G,
                                                          unsigned *__restrict__ bitmap) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  if (n >= N || (n_dev && n >= *n_dev)) return;
  int ox, oy, oz;
  int4 c = indices[n];
  if (c.x < 0 || !out_coord(G, c, k, ox, oy, oz)) return;
  long long cell = (((long long)c.x * G.out0 + ox) * G.out1 + oy) * G.out2 + oz;
  atomicOr(&bitmap[cell >> 5], 1u << (cell & 31));
}

constexpr int kScan = 1024;

__global__ __launch_bounds__(kScan) void words_count_kernel(const unsigned *__restrict__ bitmap,
                                                            long long nwords,
                                                            int *__restrict__ blk) {
  __shared__ int sm[kScan / 64];
  long long i = (long long)blockIdx.x * kScan + threadIdx.x;
  int v = i < nwords ? __popc(bitmap[i]) : 0;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    int r = 0;
    for (int k = 0; k < kScan / 64; ++k) r += sm[k];
    blk[blockIdx.x] = r;
  }
}

__global__ __launch_bounds__(kScan) void blocks_scan_kernel(int *__restrict__ blk, int nb,
                                                            int *__restrict__ total) {
  __shared__ int sm[kScan];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += kScan) {
    int i = base + threadIdx.x;
    int v = i < nb ? blk[i] : 0;
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < kScan; o <<= 1) {
      int t = threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
      __syncthreads();
      sm[threadIdx.x] += t;
      __syncthreads();
    }
    int incl = sm[threadIdx.x];
    int c = carry;
    if (i < nb) blk[i] = c + incl - v;
    __syncthreads();
    if (threadIdx.x == kScan - 1) carry = c + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}

// exclusive prefix of the per-word popcounts
__global__ __launch_bounds__(kScan) void words_prefix_kernel(const unsigned *__restrict__ bitmap,
                                                             long long nwords,
                                                             const int *__restrict__ blk_offs,
                                                             int *__restrict__ word_prefix) {
  __shared__ int sm[kScan];
  long long i = (long long)blockIdx.x * kScan + threadIdx.x;
  int v = i < nwords ? __popc(bitmap[i]) : 0;
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int o = 1; o < kScan; o <<= 1) {
    int t = threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
    __syncthreads();
    sm[threadIdx.x] += t;
    __syncthreads();
  }
  if (i < nwords) word_prefix[i] = blk_offs[blockIdx.x] + sm[threadIdx.x] - v;
}

__global__ __launch_bounds__(256) void sparse_out_indices_kernel(const unsigned *__restrict__ bitmap,
                                                                 const int *__restrict__ word_prefix,
                                                                 long long nwords, ConvGeom G,
                                                                 int max_out,
                                                                 int4 *__restrict__ out_indices) {
  long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nwords) return;
  unsigned bits = bitmap[w];
  int o = word_prefix[w];
  while (bits) {
    int bpos = __ffs(bits) - 1;
    bits &= bits - 1;
    long long cell = (w << 5) + bpos;
    int z = (int)(cell % G.out2); cell /= G.out2;
    int y = (int)(cell % G.out1); cell /= G.out1;
    int x = (int)(cell % G.out0); cell /= G.out0;
    if (o < max_out) out_indices[o] = make_int4((int)cell, x, y, z);
    ++o;
  }
}

__global__ __launch_bounds__(256) void sparse_pairs_kernel(const int4 *__restrict__ indices, int N,
                                                           ConvGeom G,
                                                           const unsigned *__restrict__ bitmap,
                                                           const int *__restrict__ word_prefix,
                                                           int ld_out, int *__restrict__ pair_fwd,
                                                           int *__restrict__ pair_bwd,
                                                           int *__restrict__ n_pairs) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = blockIdx.y;
  const long long t = (long long)k * N + n;
  bool ok = false;
  if (n < N) {
    int ox, oy, oz;
    int4 c = indices[n];
    ok = c.x >= 0 && out_coord(G, c, k, ox, oy, oz);
    int o = -1;
    if (ok) {
      long long cell = (((long long)c.x * G.out0 + ox) * G.out1 + oy) * G.out2 + oz;
      unsigned wbits = bitmap[cell >> 5];
      o = word_prefix[cell >> 5] + __popc(wbits & ((1u << (cell & 31)) - 1u));
      // ld_out may be a capacity (static capacity mode): an output row beyond it does not exist in any buffer of this
      // layer, so the pair is dropped on BOTH sides (an unclamped pair_bwd entry would make the data gradient gather
      // grad_out rows past the buffer)
      // atomicMax over the -1 pre-fill instead of a plain store: with duplicate input coordinates (malformed input; the
      // reference's own encoder test feeds them) several rows claim one slot, and the HIGHEST row wins deterministically
      if (o < ld_out) atomicMax(&pair_fwd[(size_t)k * ld_out + o], n);
      else { o = -1; ok = false; }
    }
    pair_bwd[t] = o;
  }
  unsigned long long bal = __ballot(ok);
  if (n_pairs && (threadIdx.x & 63) == 0 && bal) atomicAdd(&n_pairs[(blockIdx.x * 4 + (threadIdx.x >> 6) + k) & 63], __popcll(bal));
}

// Row-block form of sparse_pairs_kernel (same tables): workgroup = 64 input rows x (k0*k1) offset columns, a thread walks the
// k2 offsets of its column.  pair_bwd planes are written coalesced, the input rows' offset masks (the backward table's row
// masks) are assembled in LDS and leave with the identity permutation and the sort key; no global atomics.
template <int K2>
__global__ __launch_bounds__(1024) void sparse_pairs_rows_kernel(const int4 *__restrict__ indices, int N, ConvGeom G,
                                                                 const unsigned *__restrict__ bitmap,
                                                                 const int *__restrict__ word_prefix, int ld_out,
                                                                 int *__restrict__ pair_fwd, int *__restrict__ pair_bwd,
                                                                 unsigned *__restrict__ row_mask, unsigned *__restrict__ iota,
                                                                 unsigned *__restrict__ keys, int regions,
                                                                 int *__restrict__ n_pairs) {
  __shared__ unsigned smask[64];
  const int lane = threadIdx.x, ty = threadIdx.y;
  const int n = blockIdx.x * 64 + lane;
  if (ty == 0) smask[lane] = 0u;
  __syncthreads();
  const int k2 = K2 ? K2 : G.k2;
  const int i = ty / G.k1, j = ty - i * G.k1;
  int4 c = n < N ? indices[n] : make_int4(-1, 0, 0, 0);
  int ox = c.y + G.p0 - i * G.d0, oy = c.z + G.p1 - j * G.d1;
  bool xy_ok = c.x >= 0 && ox >= 0 && oy >= 0 && (ox % G.s0) == 0 && (oy % G.s1) == 0;
  ox /= G.s0; oy /= G.s1;
  xy_ok = xy_ok && ox < G.out0 && oy < G.out1;
  const long long base = (((long long)c.x * G.out0 + ox) * G.out1 + oy) * G.out2;
  unsigned bits = 0u;
  for (int l = 0; l < k2; ++l) {
    const int k = ty * k2 + l;
    int oz = c.w + G.p2 - l * G.d2;
    int o = -1;
    if (xy_ok && oz >= 0 && (oz % G.s2) == 0 && oz / G.s2 < G.out2) {
      const long long cell = base + oz / G.s2;
      const unsigned wbits = bitmap[cell >> 5];
      o = word_prefix[cell >> 5] + __popc(wbits & ((1u << (cell & 31)) - 1u));
      if (o < ld_out) {  // beyond a static capacity: the pair is dropped on both sides (see sparse_pairs_kernel)
        atomicMax(&pair_fwd[(size_t)k * ld_out + o], n);  // duplicates: highest row wins (see sparse_pairs_kernel)
        bits |= 1u << (k & 31);
      } else {
        o = -1;
      }
    }
    if (n < N) pair_bwd[(size_t)k * N + n] = o;
  }
  if (bits) atomicOr(&smask[lane], bits);
  __syncthreads();
  if (ty == 0) {
    const unsigned m = smask[lane];
    if (n < N) {
      if (row_mask) row_mask[n] = m;
      if (iota) iota[n] = (unsigned)n;
      if (keys) keys[n] = (regions > 1 ? (unsigned)(((long long)n * regions) / N) << G.KV : 0u) | m;
    }
    if (n_pairs) {
      int cnt = __popc(m);
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);
      if (lane == 0 && cnt) atomicAdd(&n_pairs[blockIdx.x & 63], cnt);
    }
  }
}

// -------------------------------------------------------------------------------- row masks
// mask[n] bit k = pair[k][n] >= 0.  Rows are then sorted by mask so that the 16 rows of an MFMA tile
// use (nearly) the same kernel offsets and whole offsets can be skipped per tile (the idea of spconv's
// mask_argsort, projects/SparseConvolution/sparse_functional.py:139-162).
__global__ __launch_bounds__(256) void row_mask_kernel(const int *__restrict__ pairs, int ld, int KV,
                                                       int n_rows, unsigned *__restrict__ mask,
                                                       unsigned *__restrict__ iota, unsigned *__restrict__ keys,
                                                       int regions) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_rows) return;
  unsigned m = 0u;
  for (int k = 0; k < KV; ++k) m |= (pairs[(size_t)k * ld + n] >= 0 ? 1u : 0u) << k;
  mask[n] = m;
  iota[n] = (unsigned)n;
  // sort key: region of the row (rows are in voxel order, so a region is a slab of space) above the mask
  if (keys) keys[n] = (unsigned)(((long long)n * regions) / n_rows) << KV | m;
}

// the *_pairs_rows_kernels have the depth k2 of the kernel compiled in for the encoder's 3 (K2 = 3); K2 = 0 reads it from G
template <typename F>
inline void dispatch_k2(int k2, F &&f) {
  k2 == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 0>{});
}

// Workspace of the strided rulebook: the bitmap over the output grid, the exclusive prefix of its words' popcounts and the
// scan's per-block sums, in this order.  bfhip_rulebook_sparse_count fills it, _out_indices and _fill read it back: the
// layout exists once, here.  workspace == nullptr: sizes only.
struct BitmapWorkspace {
  long long nwords;  // 32-cell words of the bitmap
  int nb;            // blocks of kScan words
  unsigned *bitmap = nullptr;
  int *word_prefix = nullptr, *blk = nullptr;
  BitmapWorkspace(const ConvGeom &G, void *workspace)
      : nwords(((long long)G.B * G.out0 * G.out1 * G.out2 + 31) / 32), nb(ceil_div(nwords, kScan)) {
    if (!workspace) return;
    Workspace ws(workspace, bytes());
    bitmap = ws.take<unsigned>(nwords);
    word_prefix = ws.take<int>(nwords);
    blk = ws.take<int>(nb + 1);
  }
  size_t bytes() const { return 2 * align_up((size_t)nwords * sizeof(int), 256) + align_up(((size_t)nb + 1) * sizeof(int), 256) + 256; }
};

}  // namespace
}  // namespace bfhip

using namespace bfhip;

// ------------------------------------------------------------------------------------ C ABI
BFHIP_EXPORT int bfhip_conv_out_shape(const int *in_shape, const int *ksize, const int *stride,
                                      const int *padding, const int *dilation, int *out_shape) {
  ConvGeom G;
  BFHIP_REQUIRE(make_geom(1, in_shape, ksize, stride, padding, dilation, false, G) == 0, "conv_out_shape: bad geometry");
  out_shape[0] = G.out0; out_shape[1] = G.out1; out_shape[2] = G.out2;
  return BFHIP_OK;
}

// Row masks + mask-sorted row permutation of a pair table (for tile-level offset skipping).
// rocPRIM sorts fewer than 2^20 items with a block sort + log2(n / block) merge passes (10 launches of ~5 us for the 10^5 rows
// of an encoder level).  Forcing its Onesweep radix path (merge limit 0) was measured and is slower here: the 12 sorts of a
// LiDAR pass took 1.29 ms instead of 0.52 ms (tools/sparse_micro.py), so the default configuration stays.
using RowSortConfig = rocprim::default_config;

static inline size_t sort32_bytes(int n, int bits) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs<RowSortConfig, unsigned *, unsigned *, unsigned *, unsigned *>(
      nullptr, bytes, nullptr, nullptr, nullptr, nullptr, (size_t)n, 0, bits, 0);
  return bytes;
}

BFHIP_EXPORT size_t bfhip_rulebook_sort_rows_workspace_bytes(int n_rows, int KV) {
  (void)KV;
  if (n_rows <= 0) return 256;
  return 3 * align_up((size_t)n_rows * 4, 256) + align_up(sort32_bytes(n_rows, 32), 256) + 256;
}

namespace {
// Sort key = (region of the row, mask): rows come in voxel order, so a region is a slab of space.  With the gather-GEMM's
// XCD-chunked block order each XCD then walks one region and the neighbour rows it gathers stay in its own 4 MiB L2
// (forward gather-GEMM of the encoder's layers 15-25 % faster than with a pure mask sort, tools/gemm_micro.py; 16 or
// 32 regions measured no better).  Tiles still share their offsets inside a region.
inline int sort_regions(int KV) { return KV + 3 <= 32 ? 8 : 1; }
inline int sort_bits(int KV) { return KV + (KV + 3 <= 32 ? 3 : 0); }

struct SortScratch {
  unsigned *iota, *keys_out, *keys;
  char *tmp;
  size_t tmp_bytes;
  SortScratch(void *workspace, size_t bytes, int n_rows) {
    Workspace ws(workspace, bytes);
    iota = ws.take<unsigned>(n_rows);
    keys_out = ws.take<unsigned>(n_rows);
    keys = ws.take<unsigned>(n_rows);
    tmp_bytes = sort32_bytes(n_rows, 32);
    tmp = ws.take<char>(tmp_bytes);
  }
  hipError_t sort(int n_rows, int KV, int32_t *perm, hipStream_t stream);
};

// Round 3: the row order in ONE launch.  Rows are sorted by offset mask inside consecutive chunks of kSortChunk rows (a
// chunk = a slab of space, rows being in voxel order); one 512-thread workgroup sorts one chunk in LDS (stable LSD radix,
// rocprim::block_radix_sort), instead of a device-wide sort per rulebook -- which for these 10^5-row arrays was a block sort
// plus 6-7 merge passes of ~5 us each, 12 times per LiDAR pass: 0.52 of the 1.15 ms the rulebooks cost.  The chunked order
// keeps what the device-wide (eighth of the row range, mask) order was for: tiles of 16-64 consecutive sorted rows share
// their offsets, and consecutive tiles stay in one slab of space (the gather-GEMM deals contiguous eighths of the tiles to
// the 8 XCDs).
constexpr int kSortChunk = 4096, kSortThreads = 512, kSortItems = kSortChunk / kSortThreads;

__global__ __launch_bounds__(kSortThreads) void sort_rows_chunk_kernel(const unsigned *__restrict__ keys, int n_rows, int KV,
                                                                      int *__restrict__ perm) {
  using BlockSort = rocprim::block_radix_sort<unsigned, kSortThreads, kSortItems, unsigned>;
  __shared__ typename BlockSort::storage_type storage;
  const int base = blockIdx.x * kSortChunk;
  const unsigned invalid = 1u << KV, low = invalid - 1u;  // rows beyond n_rows sort behind every real mask (KV <= 30)
  unsigned k[kSortItems], v[kSortItems];
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const int idx = base + threadIdx.x * kSortItems + i;
    k[i] = idx < n_rows ? (keys[idx] & low) : invalid;
    v[i] = (unsigned)idx;
  }
  BlockSort().sort(k, v, storage, 0, KV + 1);
#pragma unroll
  for (int i = 0; i < kSortItems; ++i) {
    const int pos = base + threadIdx.x * kSortItems + i;
    if (pos < n_rows) perm[pos] = (int)v[i];
  }
}

hipError_t SortScratch::sort(int n_rows, int KV, int32_t *perm, hipStream_t stream) {
  static const int chunked = env_int("BFHIP_SPCONV_CHUNK_SORT", 1);
  if (chunked && KV <= 30) {
    hipLaunchKernelGGL(sort_rows_chunk_kernel, dim3(ceil_div(n_rows, kSortChunk)), dim3(kSortThreads), 0, stream, keys, n_rows, KV,
                       perm);
    return hipGetLastError();
  }
  return rocprim::radix_sort_pairs<RowSortConfig>(tmp, tmp_bytes, keys, keys_out, iota, (unsigned *)perm, (size_t)n_rows, 0, sort_bits(KV), stream);
}
}  // namespace

// SubM rulebook.  row_mask / perm (optional, KV <= 32): the offset masks of the rows and their (region, mask)-sorted order, as
// bfhip_rulebook_sort_rows(pair_fwd) would give them, produced by the same launch that fills the table.
BFHIP_EXPORT size_t bfhip_rulebook_subm_workspace_bytes(int N) {
  return align_up((size_t)table_cap(N > 0 ? N : 1) * sizeof(int2), 256) + bfhip_rulebook_sort_rows_workspace_bytes(N, 27) + 256;
}

BFHIP_EXPORT int bfhip_rulebook_subm(const int32_t *indices, int N, int B, const int *in_shape,
                                     const int *ksize, const int *dilation, int32_t *pair_fwd,
                                     int32_t *n_pairs_dev, uint32_t *row_mask, int32_t *perm, void *workspace,
                                     size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ConvGeom G;
  BFHIP_REQUIRE(N >= 0, "rulebook_subm: N < 0");
  BFHIP_REQUIRE(make_geom(B, in_shape, ksize, nullptr, nullptr, dilation, true, G) == 0,
                "rulebook_subm: bad geometry (B*X*Y*Z must be < 2^31, kernel volume <= 64)");
  BFHIP_REQUIRE(!(row_mask || perm) || G.KV <= 32, "rulebook_subm: row masks need a kernel volume <= 32");
  BFHIP_REQUIRE(!perm || row_mask, "rulebook_subm: perm without row_mask");
  if (n_pairs_dev && hipMemsetAsync(n_pairs_dev, 0, 64 * sizeof(int), stream) != hipSuccess) return check_launch("rulebook_subm memset");
  if (N == 0) return BFHIP_OK;
  BFHIP_REQUIRE(indices && pair_fwd && ((uintptr_t)indices % 16) == 0, "rulebook_subm: null/unaligned pointer");
  BFHIP_REQUIRE_WORKSPACE(workspace, workspace_bytes, bfhip_rulebook_subm_workspace_bytes(N), "rulebook_subm");
  Workspace ws(workspace, workspace_bytes);
  unsigned cap = table_cap(N);
  int2 *table = ws.take<int2>(cap);
  size_t sort_bytes = bfhip_rulebook_sort_rows_workspace_bytes(N, G.KV);
  SortScratch ss(ws.take<char>(sort_bytes), sort_bytes, N);
  ProfScope ps;
  prof_begin(BFHIP_OP_RULEBOOK, stream, &ps);
  hipLaunchKernelGGL(fill_pair_kernel, dim3(ceil_div(cap, 256)), dim3(256), 0, stream, table, (int)cap);
  hipLaunchKernelGGL(subm_insert_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, stream, (const int4 *)indices, N, G,
                     table, cap - 1);
  hipError_t e = hipSuccess;
  if (G.k0 * G.k1 <= 16 && G.KV <= 32) {
    dim3 block(64, G.k0 * G.k1);
    unsigned *iota = perm ? ss.iota : nullptr, *keys = perm ? ss.keys : nullptr;
    dispatch_k2(G.k2, [&](auto k2) {
      hipLaunchKernelGGL(subm_pairs_rows_kernel<k2.value>, dim3(ceil_div(N, 64)), block, 0, stream,
                         (const int4 *)indices, N, G, table, cap - 1, pair_fwd, row_mask, iota, keys, sort_regions(G.KV),
                         n_pairs_dev);
    });
  } else {
    // wide kernels: one thread per (row, offset) over the lower half of the offsets, mirrored writes (pre-filled table)
    (void)hipMemsetAsync(pair_fwd, 0xff, (size_t)G.KV * N * sizeof(int), stream);
    const int symmetric = (G.k0 % 2 == 1) && (G.k1 % 2 == 1) && (G.k2 % 2 == 1);
    const int nk = symmetric ? G.KV / 2 + 1 : G.KV;
    hipLaunchKernelGGL(subm_pairs_kernel, dim3(ceil_div(N, 256), nk), dim3(256), 0, stream, (const int4 *)indices, N,
                       G, table, cap - 1, pair_fwd, n_pairs_dev, symmetric);
    if (row_mask)
      hipLaunchKernelGGL(row_mask_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, stream, pair_fwd, N, G.KV, N, row_mask, ss.iota,
                         ss.keys, sort_regions(G.KV));
  }
  if (perm) e = ss.sort(N, G.KV, perm, stream);
  prof_end(&ps);
  if (e != hipSuccess) { set_error("rulebook_subm: sort: %s", hipGetErrorString(e)); return BFHIP_E_LAUNCH; }
  return check_launch("rulebook_subm");
}

// Strided rulebook, two phases (the output row count must reach the host to size the outputs):
//   count: bitmap over the output grid + prefix popcounts -> counts_dev[0] = N_out
//   fill : out_indices (ascending linear order), pair_fwd[KV, ld_out], pair_bwd[KV, N],
//          sum(counts_dev[1..64]) = pairs (64 spread counters: one hot word would serialise the atomics)
// The workspace must be kept untouched between the two calls.
BFHIP_EXPORT size_t bfhip_rulebook_sparse_workspace_bytes(int B, const int *in_shape, const int *ksize,
                                                          const int *stride, const int *padding,
                                                          const int *dilation) {
  ConvGeom G;
  if (make_geom(B, in_shape, ksize, stride, padding, dilation, false, G) != 0) return 0;
  return BitmapWorkspace(G, nullptr).bytes();
}

BFHIP_EXPORT int bfhip_rulebook_sparse_count(const int32_t *indices, int N, const int32_t *n_in_dev, int B,
                                             const int *in_shape, const int *ksize, const int *stride,
                                             const int *padding, const int *dilation, int32_t *counts_dev,
                                             void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ConvGeom G;
  BFHIP_REQUIRE(N >= 0, "rulebook_sparse: N < 0");
  BFHIP_REQUIRE(make_geom(B, in_shape, ksize, stride, padding, dilation, false, G) == 0, "rulebook_sparse: bad geometry");
  BFHIP_REQUIRE(counts_dev && (N == 0 || (indices && ((uintptr_t)indices % 16) == 0)), "rulebook_sparse: null/unaligned pointer");
  const size_t need = BitmapWorkspace(G, nullptr).bytes();
  // (this message carries the sizes, so it is not a BFHIP_REQUIRE_WORKSPACE)
  if (workspace_bytes < need || !workspace) { set_error("rulebook_sparse: workspace too small (%zu < %zu)", workspace_bytes, need); return BFHIP_E_WORKSPACE; }
  const BitmapWorkspace bw(G, workspace);
  ProfScope ps;
  prof_begin(BFHIP_OP_RULEBOOK, stream, &ps);
  (void)hipMemsetAsync(bw.bitmap, 0, bw.nwords * sizeof(unsigned), stream);
  (void)hipMemsetAsync(counts_dev, 0, 65 * sizeof(int), stream);
  if (N > 0) {
    hipLaunchKernelGGL(sparse_mark_kernel, dim3(ceil_div(N, 256), G.KV), dim3(256), 0, stream, (const int4 *)indices, N, n_in_dev, G, bw.bitmap);
  }
  hipLaunchKernelGGL(words_count_kernel, dim3(bw.nb), dim3(kScan), 0, stream, bw.bitmap, bw.nwords, bw.blk);
  hipLaunchKernelGGL(blocks_scan_kernel, dim3(1), dim3(kScan), 0, stream, bw.blk, bw.nb, counts_dev);
  hipLaunchKernelGGL(words_prefix_kernel, dim3(bw.nb), dim3(kScan), 0, stream, bw.bitmap, bw.nwords, bw.blk, bw.word_prefix);
  prof_end(&ps);
  return check_launch("rulebook_sparse_count");
}

// Output coordinates of a counted layer into a buffer of `cap` rows, without knowing N_out on the host (rows beyond cap are
// dropped; the caller compares counts_dev[0] with cap after its single read).  Lets a chain of strided layers be counted
// back to back: the next layer's bfhip_rulebook_sparse_count takes this buffer with n_in_dev = counts_dev of this one.
BFHIP_EXPORT int bfhip_rulebook_sparse_out_indices(int B, const int *in_shape, const int *ksize, const int *stride,
                                                   const int *padding, const int *dilation, int cap,
                                                   int32_t *out_indices, void *workspace, size_t workspace_bytes,
                                                   void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ConvGeom G;
  BFHIP_REQUIRE(make_geom(B, in_shape, ksize, stride, padding, dilation, false, G) == 0, "rulebook_sparse_out_indices: bad geometry");
  BFHIP_REQUIRE(cap > 0 && out_indices && ((uintptr_t)out_indices % 16) == 0, "rulebook_sparse_out_indices: bad output buffer");
  BFHIP_REQUIRE_WORKSPACE(workspace, workspace_bytes, BitmapWorkspace(G, nullptr).bytes(), "rulebook_sparse_out_indices");
  const BitmapWorkspace bw(G, workspace);
  ProfScope ps;
  prof_begin(BFHIP_OP_RULEBOOK, stream, &ps);
  hipLaunchKernelGGL(sparse_out_indices_kernel, dim3(ceil_div(bw.nwords, 256)), dim3(256), 0, stream, bw.bitmap, bw.word_prefix,
                     bw.nwords, G, cap, (int4 *)out_indices);
  prof_end(&ps);
  return check_launch("rulebook_sparse_out_indices");
}

// mask_fwd / perm_fwd (output rows) and mask_bwd / perm_bwd (input rows), optional, KV <= 32: what bfhip_rulebook_sort_rows gives
// for pair_fwd and pair_bwd; the backward ones leave with the pair kernel itself.  sort_workspace:
// bfhip_rulebook_sort_rows_workspace_bytes(max(N, n_out), KV) bytes (only needed with the masks).
BFHIP_EXPORT int bfhip_rulebook_sparse_fill(const int32_t *indices, int N, int B, const int *in_shape,
                                            const int *ksize, const int *stride, const int *padding,
                                            const int *dilation, int n_out, int32_t *out_indices,
                                            int32_t *pair_fwd, int32_t *pair_bwd, int32_t *counts_dev,
                                            uint32_t *mask_fwd, int32_t *perm_fwd, uint32_t *mask_bwd, int32_t *perm_bwd,
                                            void *sort_workspace, size_t sort_workspace_bytes,
                                            void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ConvGeom G;
  BFHIP_REQUIRE(make_geom(B, in_shape, ksize, stride, padding, dilation, false, G) == 0, "rulebook_sparse: bad geometry");
  BFHIP_REQUIRE(N >= 0 && n_out >= 0, "rulebook_sparse_fill: bad sizes");
  if (N == 0 || n_out == 0) return BFHIP_OK;
  BFHIP_REQUIRE(indices && out_indices && pair_fwd && pair_bwd, "rulebook_sparse_fill: null pointer");
  BFHIP_REQUIRE(((uintptr_t)indices % 16) == 0 && ((uintptr_t)out_indices % 16) == 0, "rulebook_sparse_fill: indices must be 16-byte aligned");
  const bool masks = mask_fwd || mask_bwd;
  BFHIP_REQUIRE(!masks || (mask_fwd && mask_bwd && G.KV <= 32), "rulebook_sparse_fill: row masks come in pairs and need a kernel volume <= 32");
  BFHIP_REQUIRE((!perm_fwd && !perm_bwd) || (masks && perm_fwd && perm_bwd), "rulebook_sparse_fill: perms need the masks (and come in pairs)");
  BFHIP_REQUIRE_WORKSPACE(workspace, workspace_bytes, BitmapWorkspace(G, nullptr).bytes(), "rulebook_sparse_fill");
  const int n_sort = N > n_out ? N : n_out;
  if (masks && (!sort_workspace || sort_workspace_bytes < bfhip_rulebook_sort_rows_workspace_bytes(n_sort, G.KV))) {
    set_error("rulebook_sparse_fill: sort workspace too small");  // (its own wording, so not a BFHIP_REQUIRE_WORKSPACE)
    return BFHIP_E_WORKSPACE;
  }
  const BitmapWorkspace bw(G, workspace);
  int *n_pairs = counts_dev ? counts_dev + 1 : nullptr;
  ProfScope ps;
  prof_begin(BFHIP_OP_RULEBOOK, stream, &ps);
  (void)hipMemsetAsync(pair_fwd, 0xff, (size_t)G.KV * n_out * sizeof(int), stream);
  // n_out may be a capacity (true count only on the device): rows the kernel below does not reach stay inactive (-1)
  (void)hipMemsetAsync(out_indices, 0xff, (size_t)n_out * sizeof(int4), stream);
  hipLaunchKernelGGL(sparse_out_indices_kernel, dim3(ceil_div(bw.nwords, 256)), dim3(256), 0, stream, bw.bitmap, bw.word_prefix,
                     bw.nwords, G, n_out, (int4 *)out_indices);
  hipError_t e = hipSuccess;
  if (G.k0 * G.k1 <= 16 && G.KV <= 32) {
    unsigned *iota = nullptr, *keys = nullptr;
    SortScratch sb(masks ? sort_workspace : nullptr, masks ? sort_workspace_bytes : 0, masks ? N : 0);
    if (perm_bwd) { iota = sb.iota; keys = sb.keys; }
    dim3 block(64, G.k0 * G.k1);
    dispatch_k2(G.k2, [&](auto k2) {
      hipLaunchKernelGGL(sparse_pairs_rows_kernel<k2.value>, dim3(ceil_div(N, 64)), block, 0, stream,
                         (const int4 *)indices, N, G, bw.bitmap, bw.word_prefix, n_out, pair_fwd, pair_bwd, mask_bwd, iota, keys,
                         sort_regions(G.KV), n_pairs);
    });
    if (perm_bwd) e = sb.sort(N, G.KV, perm_bwd, stream);
  } else {
    hipLaunchKernelGGL(sparse_pairs_kernel, dim3(ceil_div(N, 256), G.KV), dim3(256), 0, stream, (const int4 *)indices, N, G,
                       bw.bitmap, bw.word_prefix, n_out, pair_fwd, pair_bwd, n_pairs);
    if (masks) {
      SortScratch sb(sort_workspace, sort_workspace_bytes, N);
      hipLaunchKernelGGL(row_mask_kernel, dim3(ceil_div(N, 256)), dim3(256), 0, stream, pair_bwd, N, G.KV, N, mask_bwd, sb.iota,
                         sb.keys, sort_regions(G.KV));
      if (perm_bwd) e = sb.sort(N, G.KV, perm_bwd, stream);
    }
  }
  if (masks && e == hipSuccess) {
    SortScratch sf(sort_workspace, sort_workspace_bytes, n_out);
    hipLaunchKernelGGL(row_mask_kernel, dim3(ceil_div(n_out, 256)), dim3(256), 0, stream, pair_fwd, n_out, G.KV, n_out, mask_fwd,
                       sf.iota, sf.keys, sort_regions(G.KV));
    if (perm_fwd) e = sf.sort(n_out, G.KV, perm_fwd, stream);
  }
  prof_end(&ps);
  if (e != hipSuccess) { set_error("rulebook_sparse_fill: sort: %s", hipGetErrorString(e)); return BFHIP_E_LAUNCH; }
  return check_launch("rulebook_sparse_fill");
}

BFHIP_EXPORT int bfhip_rulebook_sort_rows(const int32_t *pairs, int ld, int KV, int n_rows, uint32_t *row_mask,
                                          int32_t *perm, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BFHIP_REQUIRE(KV > 0 && KV <= 32 && n_rows >= 0 && ld >= n_rows, "rulebook_sort_rows: bad sizes");
  if (n_rows == 0) return BFHIP_OK;
  BFHIP_REQUIRE(pairs && row_mask, "rulebook_sort_rows: null pointer");
  BFHIP_REQUIRE_WORKSPACE(workspace, workspace_bytes, bfhip_rulebook_sort_rows_workspace_bytes(n_rows, KV), "rulebook_sort_rows");
  SortScratch sc(workspace, workspace_bytes, n_rows);
  ProfScope ps;
  prof_begin(BFHIP_OP_RULEBOOK, stream, &ps);
  hipLaunchKernelGGL(row_mask_kernel, dim3(ceil_div(n_rows, 256)), dim3(256), 0, stream, pairs, ld, KV, n_rows, row_mask, sc.iota,
                     sc.keys, sort_regions(KV));
  hipError_t e = hipSuccess;
  if (perm)  // perm == NULL: masks only
    e = sc.sort(n_rows, KV, perm, stream);
  prof_end(&ps);
  if (e != hipSuccess) { set_error("rulebook_sort_rows: sort: %s", hipGetErrorString(e)); return BFHIP_E_LAUNCH; }
  return check_launch("rulebook_sort_rows");
}

// Debug guard of the gather kernels' operands (they dereference pairs[k*ld + perm[i]] and in + pairs[..]*Kdim unchecked):
// status[0] = pair entries outside [-1, n_src), status[1] = perm entries outside [0, n_rows), status[2] = rows that do
// not occur exactly once in perm, status[3] = rows whose row_mask disagrees with the table.  `seen` = i32[n_rows], zeroed.
namespace {
__global__ __launch_bounds__(256) void rulebook_validate_kernel(const int *__restrict__ pairs, int ld, int KV, int n_rows,
                                                                int n_src, const int *__restrict__ perm,
                                                                const unsigned *__restrict__ row_mask,
                                                                int *__restrict__ seen, int *__restrict__ status) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= n_rows) return;
  unsigned m = 0u;
  int bad = 0;
  for (int k = 0; k < KV; ++k) {
    const int v = pairs[(size_t)k * ld + n];
    if (v < -1 || v >= n_src) ++bad;
    if (v >= 0 && k < 32) m |= 1u << k;
  }
  if (bad) atomicAdd(&status[0], bad);
  if (row_mask && KV <= 32 && row_mask[n] != m) atomicAdd(&status[3], 1);
  if (perm) {
    const int p = perm[n];
    if (p < 0 || p >= n_rows) atomicAdd(&status[1], 1);
    else atomicAdd(&seen[p], 1);
  }
}

__global__ __launch_bounds__(256) void rulebook_validate_perm_kernel(const int *__restrict__ seen, int n_rows,
                                                                     int *__restrict__ status) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n < n_rows && seen[n] != 1) atomicAdd(&status[2], 1);
}
}  // namespace

BFHIP_EXPORT size_t bfhip_rulebook_validate_workspace_bytes(int n_rows) {
  return align_up((size_t)(n_rows > 0 ? n_rows : 1) * sizeof(int), 256) + 256;
}

BFHIP_EXPORT int bfhip_rulebook_validate(const int32_t *pairs, int ld, int KV, int n_rows, int n_src, const int32_t *perm,
                                         const uint32_t *row_mask, int32_t *status_dev, void *workspace,
                                         size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BFHIP_REQUIRE(KV > 0 && KV <= 64 && n_rows >= 0 && ld >= n_rows && n_src >= 0, "rulebook_validate: bad sizes");
  BFHIP_REQUIRE(status_dev, "rulebook_validate: status_dev is null");
  if (hipMemsetAsync(status_dev, 0, 4 * sizeof(int), stream) != hipSuccess) return check_launch("rulebook_validate memset");
  if (n_rows == 0) return BFHIP_OK;
  BFHIP_REQUIRE(pairs, "rulebook_validate: null pointer");
  BFHIP_REQUIRE_WORKSPACE(workspace, workspace_bytes, bfhip_rulebook_validate_workspace_bytes(n_rows), "rulebook_validate");
  int *seen = (int *)workspace;
  if (perm && hipMemsetAsync(seen, 0, (size_t)n_rows * sizeof(int), stream) != hipSuccess) return check_launch("rulebook_validate memset");
  hipLaunchKernelGGL(rulebook_validate_kernel, dim3(ceil_div(n_rows, 256)), dim3(256), 0, stream, pairs, ld, KV, n_rows, n_src,
                     perm, row_mask, seen, status_dev);
  if (perm)
    hipLaunchKernelGGL(rulebook_validate_perm_kernel, dim3(ceil_div(n_rows, 256)), dim3(256), 0, stream, seen, n_rows, status_dev);
  return check_launch("rulebook_validate");
}
