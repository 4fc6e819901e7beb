// points_aug.hip -- the point half of the LiDAR augmentation chain on the device (gfx950), for a whole batch at once:
// GlobalRotScaleTrans (rotate, then translate and scale in either order), RandomFlip3D (sign flips), PointsRangeFilter (strict
// > min / < max on the transformed xyz, order-preserving compaction) and PointShuffle (a keyed bijection of [0, kept)).
//
// The arithmetic is the one points_aug.torch_points_aug defines: every product and sum a separate float32 operation
// (__fmul_rn / __fadd_rn: nothing contracts them), x' = (x r00 + y r10) + z r20, so the kernels and the torch restatement agree
// bit for bit.  Columns 3 .. C-1 are copied.
//
// Three launches per kMaxSamples samples, count -> scan -> ranked write (voxelize.hip 2a-2c):
//   1. points_count_kernel: one workgroup of kBlock threads per kBlock consecutive rows of one sample.  The rows (C floats,
//      12-32 B, not 16-byte aligned in general) are one contiguous run of kBlock * C dwords: consecutive lanes load consecutive
//      dwords into LDS, then thread t takes row t from there.  Transform, test, wave __ballot / __popcll -> one count per block.
//   2. points_scan_kernel: ONE workgroup scans the block counts of every sample in turn (exclusive, in place) and writes the
//      sample's kept count.
//   3. points_write_kernel: the same load, transform and test; rank = block offset + wave offset + lanes below.  Shuffle off: the
//      block's kept rows are one contiguous run of the output -- compacted in LDS, stored dword by dword.  Shuffle on: row
//      perm(rank) of the sample, C stores by the owning thread (a scatter by nature).
// No launch waits on another block of the same launch.  Sample descriptors travel in the kernel arguments.
//
// The three entries (bfhip_points_aug, _paste, _sweeps) share one host driver, run_points_aug: the checks of a whole batch, the
// descriptor copy and the three launches per chunk are written once; an entry only says which of the two tables below it
// brings, and those select among the four instantiations <HasPaste, HasSweeps> of kernels 1 and 3.
//
// ObjectSample's paste (bfhip_points_aug_paste) is a compile-time variant of kernels 1 and 3, HasPaste; the instantiation
// without it is what bfhip_points_aug launches.  With it a sample's row space is [m pasted rows ; n original rows]:
// the pasted rows and the sample's K x 6 plane equations (K <= kMaxBoxes) live in device memory, their pointers and counts
// travel beside the sample descriptors (Args + PasteArgs: 2.4 KB of the 4 KB of kernel arguments), stage_rows_paste fills
// the tile from both sources when a block straddles the boundary and puts the plane table into LDS (6 KB at the cap) once
// per block.  An original row is kept when it is inside no box -- for some plane ((x n0 + y n1) + z n2) + d >= 0, on the
// UNtransformed xyz, unfused like the rotation; all lanes of a wave read the same plane (an LDS broadcast) and leave a box at its
// first such plane -- and then passes the chain above; pasted rows skip the box test.  Scan, ranks and shuffle do not change:
// they see one sample of m + n rows.
//
// LoadPointsFromMultiSweeps (bfhip_points_aug_sweeps) is a second compile-time variant, HasSweeps, alone or with HasPaste; the
// instantiations without it are what the two entries above launch.  A sample's own rows are then [keyframe ; sweep
// 1 ; ... ; sweep S], still ONE contiguous buffer (stage_rows / stage_rows_paste do not change), cut into at most kMaxSegments
// segments {first row, flags, dt, radius, double m[9], double t[3]} (112 B).  The tables live in device memory -- 16 x 16 of
// them would not fit the kernel arguments -- and only a pointer and a count per sample travel beside Args / PasteArgs; a block
// puts its sample's table into LDS (1.75 KB at the cap) with the rows.  Thread t finds its row's segment by a walk over the
// boundaries in LDS (a block generally straddles some), drops the row when |x| < radius and |y| < radius on the raw floats,
// multiplies by lidar2sensor in float64 (__dmul_rn / __dadd_rn: (x m0j + y m1j) + z m2j, rounded to float32, minus t_j in
// float64, rounded again -- the reference's numpy expression, operation for operation) and writes dt into column 4 of its row in
// the tile.  The box test of a paste then runs on these xyz.  Pasted rows are in no segment.
//
// perm(r), n = kept count: a balanced Feistel network of kRounds rounds on 2 * h bits, h = max(1, ceil(bitlength(n - 1) / 2)),
// walked until the value is below n (cycle walking: the network is a bijection of [0, 4^h) whatever the round function, so the
// walk follows the cycle of r, which comes back to r < n: it terminates, and the restriction is a bijection of [0, n)).  Round
// i: (L, R) <- (R, L ^ (mix(R + key_i) & (2^h - 1))), mix the 32-bit finaliser below; at the end value = L << h | R.
#include "common.h"
#include "points_tile.h"

namespace bfhip {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxC = 8;
constexpr int kMaxSamples = 16;  // descriptors per launch (kernel arguments)
constexpr int kRounds = BFHIP_POINTS_AUG_ROUNDS;
constexpr int kScanBlock = 1024;
constexpr int kMaxBoxes = 64;    // pasted boxes per sample: the plane table is kMaxBoxes * 24 floats of LDS (6 KB)

enum : int { kHasRTS = 1, kScaleFirst = 2, kFlipY = 4, kFlipX = 8, kHasRange = 16, kShuffle = 32 };

struct Sample {
  const float *src;
  int n;
  int block0;     // first block of the sample in the launch
  int row0;       // first output row of the sample's region
  int flags;
  float r[9], t[3], s, range[6];
  uint32_t key[kRounds];
};
struct Args {
  Sample s[kMaxSamples];
  int n_samples, C;
};
// the paste of one sample: m rows in front of the sample's own, K boxes as K x 6 plane equations (both in device memory)
struct Paste {
  const float *pts;
  const float *planes;
  int m, K;
};
struct PasteArgs {
  Paste p[kMaxSamples];
};
// the sweep step of one sample: nseg segments in device memory (nseg = 0: the sample has none)
constexpr int kMaxSegments = BFHIP_POINTS_AUG_MAX_SEGMENTS;
enum : int { kRemoveClose = 1, kToSensor = 2 };
using Segment = bfhip_points_aug_segment;
constexpr int kSegmentDwords = sizeof(Segment) / 4;
static_assert(sizeof(Segment) == 112 && alignof(Segment) == 8, "segment layout: 4 dwords, then 12 doubles");
struct Sweeps {
  const Segment *seg;
  int nseg;
};
struct SweepArgs {
  Sweeps w[kMaxSamples];
};
static_assert(sizeof(Args) + sizeof(PasteArgs) + sizeof(SweepArgs) + 3 * sizeof(void *) <= 4096,
              "kernel arguments: HIP passes at most 4 KB");

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x = ((x >> 16) ^ x) * 0x45d9f3bu;
  x = ((x >> 16) ^ x) * 0x45d9f3bu;
  return (x >> 16) ^ x;
}

__device__ __forceinline__ uint32_t permute(uint32_t r, uint32_t n, const uint32_t *key) {
  int bits = 32 - __clz((int)(n - 1));  // n >= 1; n = 1: __clz(0) = 32
  int h = (bits + 1) >> 1;
  h = h < 1 ? 1 : h;
  const uint32_t mask = (1u << h) - 1u;
  uint32_t v = r;
  do {
    uint32_t L = v >> h, R = v & mask;
#pragma unroll
    for (int i = 0; i < kRounds; ++i) {
      const uint32_t f = mix32(R + key[i]) & mask;
      const uint32_t nr = L ^ f;
      L = R;
      R = nr;
    }
    v = (L << h) | R;
  } while (v >= n);
  return v;
}

__device__ __forceinline__ int sample_of_block(const Args &a, int b) {
  int s = 0;
  for (int i = 1; i < a.n_samples; ++i)
    if (a.s[i].block0 <= b) s = i;  // block0 does not decrease; empty samples share their successor's: the last one wins
  return s;
}

// transformed xyz of one row and whether it is kept
__device__ __forceinline__ bool transform(const Sample &sp, float &x, float &y, float &z) {
  const int f = sp.flags;
  if (f & kHasRTS) {
    const float nx = __fadd_rn(__fadd_rn(__fmul_rn(x, sp.r[0]), __fmul_rn(y, sp.r[3])), __fmul_rn(z, sp.r[6]));
    const float ny = __fadd_rn(__fadd_rn(__fmul_rn(x, sp.r[1]), __fmul_rn(y, sp.r[4])), __fmul_rn(z, sp.r[7]));
    const float nz = __fadd_rn(__fadd_rn(__fmul_rn(x, sp.r[2]), __fmul_rn(y, sp.r[5])), __fmul_rn(z, sp.r[8]));
    if (f & kScaleFirst) {
      x = __fadd_rn(__fmul_rn(nx, sp.s), sp.t[0]);
      y = __fadd_rn(__fmul_rn(ny, sp.s), sp.t[1]);
      z = __fadd_rn(__fmul_rn(nz, sp.s), sp.t[2]);
    } else {
      x = __fmul_rn(__fadd_rn(nx, sp.t[0]), sp.s);
      y = __fmul_rn(__fadd_rn(ny, sp.t[1]), sp.s);
      z = __fmul_rn(__fadd_rn(nz, sp.t[2]), sp.s);
    }
  }
  if (f & kFlipY) y = -y;
  if (f & kFlipX) x = -x;
  if (f & kHasRange)
    return x > sp.range[0] && y > sp.range[1] && z > sp.range[2] && x < sp.range[3] && y < sp.range[4] && z < sp.range[5];
  return true;
}

// stage_rows for a block of a sample with a paste: rows [first, first + rows) of the row space [m pasted rows ; original
// rows] (the boundary generally falls inside the block's run of dwords), and the sample's plane table
__device__ __forceinline__ void stage_rows_paste(const Paste &pd, const float *__restrict__ src, long long first, int rows, int C,
                                                 float *tile, float *planes) {
  const int nd = rows * C;
  const long long b = ((long long)pd.m - first) * C;  // dwords of the run that come from the pasted rows
  const int bd = b < 0 ? 0 : (b > nd ? nd : (int)b);
  const long long p0 = first * C, s0 = (first - pd.m) * C;  // s0 + d >= 0 wherever d >= bd
  for (int d = threadIdx.x; d < nd; d += kBlock) tile[d] = d < bd ? pd.pts[p0 + d] : src[s0 + d];
  const int np = pd.K * kPlaneFloats;
  for (int d = threadIdx.x; d < np; d += kBlock) planes[d] = pd.planes[d];
}

// is the untransformed (x, y, z) inside any of the K boxes?  planes: K x 6 x (n0, n1, n2, d) in LDS; every lane of a wave reads
// the same plane at the same time (a broadcast), and a box is left at its first plane with sign >= 0
__device__ __forceinline__ bool inside_any_box(const float *planes, int K, float x, float y, float z) {
  for (int j = 0; j < K; ++j) {
    const float *pl = planes + j * kPlaneFloats;
    bool inside = true;
    for (int k = 0; k < 6; ++k) {
      if (!(plane_sign(pl + 4 * k, x, y, z) < 0.f)) {  // NaN: left
        inside = false;
        break;
      }
    }
    if (inside) return true;
  }
  return false;
}

// the sample's segment table into LDS as dwords (with the rows, before the block's barrier); fields are read back by dword
__device__ __forceinline__ void stage_segments(const Sweeps &sw, uint32_t *segs) {
  const uint32_t *src = (const uint32_t *)sw.seg;
  const int nd = sw.nseg * kSegmentDwords;
  for (int d = threadIdx.x; d < nd; d += kBlock) segs[d] = src[d];
}

// double k of a staged segment (m[0..8], t[0..2]): dwords 4 + 2 k (low half) and 5 + 2 k
__device__ __forceinline__ double segment_double(const uint32_t *sg, int k) {
  return __hiloint2double((int)sg[5 + 2 * k], (int)sg[4 + 2 * k]);
}

// The sweep step of row r of the sample's own rows: its segment by a walk over the boundaries (they do not decrease; an empty
// segment shares its successor's: the last one wins), the remove-close test on the raw x, y, xyz through lidar2sensor in float64,
// and the segment's dt.  False: the row is removed.
__device__ __forceinline__ bool sweep_row(const uint32_t *segs, int nseg, long long r, float &x, float &y, float &z, float &dt) {
  int s = 0;
  for (int k = 1; k < nseg; ++k)
    if ((int)segs[k * kSegmentDwords] <= r) s = k;
  const uint32_t *sg = segs + s * kSegmentDwords;
  const int f = (int)sg[1];
  const float radius = __uint_as_float(sg[3]);
  dt = __uint_as_float(sg[2]);
  const bool close = (f & kRemoveClose) && fabsf(x) < radius && fabsf(y) < radius;
  if (f & kToSensor) {
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    float v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float w = (float)__dadd_rn(__dadd_rn(__dmul_rn(dx, segment_double(sg, j)), __dmul_rn(dy, segment_double(sg, 3 + j))),
                                       __dmul_rn(dz, segment_double(sg, 6 + j)));
      v[j] = (float)__dadd_rn((double)w, -segment_double(sg, 9 + j));
    }
    x = v[0], y = v[1], z = v[2];
  }
  return !close;
}

// One block of the count kernel.  HasSweeps: the sample's own rows go through sweep_row first (segment table in LDS once per
// block; a removed row is not kept).  HasPaste: the sample's row space is its m pasted rows, then its n original rows (sp.n = m +
// n), the block's run of rows may straddle the boundary, the plane table goes to LDS once per block and an original row inside
// any box is not kept.
template <bool HasPaste, bool HasSweeps>
__device__ __forceinline__ void count_block(const Args &a, const PasteArgs *pa, const SweepArgs *wa,
                                            int *__restrict__ block_counts) {
  __shared__ float tile[kBlock * kMaxC];
  __shared__ int wsum[kWaves];
  __shared__ float planes[HasPaste ? kMaxBoxes * kPlaneFloats : 1];  // without a paste: unused, and gone from the kernel
  __shared__ uint32_t segs[HasSweeps ? kMaxSegments * kSegmentDwords : 1];
  const int si = sample_of_block(a, blockIdx.x);
  const Sample &sp = a.s[si];
  const long long first = (long long)(blockIdx.x - sp.block0) * kBlock;
  const int rows = sp.n - first < kBlock ? (int)(sp.n - first) : kBlock;
  if constexpr (HasPaste) {
    stage_rows_paste(pa->p[si], sp.src, first, rows, a.C, tile, planes);
  } else {
    stage_rows<kBlock>(sp.src, first, rows, a.C, tile);
  }
  if constexpr (HasSweeps) stage_segments(wa->w[si], segs);
  __syncthreads();
  const int t = threadIdx.x;
  bool keep = false;
  if (t < rows) {
    float x = tile[t * a.C], y = tile[t * a.C + 1], z = tile[t * a.C + 2];
    bool dropped = false;
    if constexpr (HasSweeps) {
      long long r = first + t;  // among the sample's own rows
      if constexpr (HasPaste) r -= pa->p[si].m;
      float dt;
      if (wa->w[si].nseg > 0 && r >= 0) dropped = !sweep_row(segs, wa->w[si].nseg, r, x, y, z, dt);
    }
    if constexpr (HasPaste) dropped = dropped || (first + t >= pa->p[si].m && inside_any_box(planes, pa->p[si].K, x, y, z));
    keep = transform(sp, x, y, z);
    if constexpr (HasPaste || HasSweeps) keep = keep && !dropped;
  }
  const unsigned long long bal = __ballot(keep);
  if ((t & (kWave - 1)) == 0) wsum[t / kWave] = __popcll(bal);
  __syncthreads();
  if (t == 0) {
    int tot = 0;
    for (int k = 0; k < kWaves; ++k) tot += wsum[k];
    block_counts[blockIdx.x] = tot;
  }
}

__global__ __launch_bounds__(kBlock) void points_count_kernel(Args a, int *__restrict__ block_counts) {
  count_block<false, false>(a, nullptr, nullptr, block_counts);
}

__global__ __launch_bounds__(kBlock) void points_count_paste_kernel(Args a, PasteArgs pa, int *__restrict__ block_counts) {
  count_block<true, false>(a, &pa, nullptr, block_counts);
}

__global__ __launch_bounds__(kBlock) void points_count_sweeps_kernel(Args a, SweepArgs wa, int *__restrict__ block_counts) {
  count_block<false, true>(a, nullptr, &wa, block_counts);
}

__global__ __launch_bounds__(kBlock) void points_count_paste_sweeps_kernel(Args a, PasteArgs pa, SweepArgs wa,
                                                                           int *__restrict__ block_counts) {
  count_block<true, true>(a, &pa, &wa, block_counts);
}

// exclusive scan of each sample's block counts, in place; kept[s] = the sample's total
__global__ __launch_bounds__(kScanBlock) void points_scan_kernel(Args a, int total_blocks, int *__restrict__ block_counts,
                                                                 int *__restrict__ kept) {
  __shared__ int wtot[kScanBlock / kWave];
  __shared__ int carry;
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  for (int s = 0; s < a.n_samples; ++s) {
    const int b0 = a.s[s].block0;
    const int b1 = s + 1 < a.n_samples ? a.s[s + 1].block0 : total_blocks;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = b0; base < b1; base += kScanBlock) {
      const int i = base + t;
      const int v = i < b1 ? block_counts[i] : 0;
      int incl = v;
      for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
      }
      if (lane == kWave - 1) wtot[wv] = incl;
      __syncthreads();
      int woff = 0;
      for (int k = 0; k < wv; ++k) woff += wtot[k];
      const int c = carry;
      if (i < b1) block_counts[i] = c + woff + incl - v;
      __syncthreads();
      if (t == kScanBlock - 1) carry = c + woff + incl;
      __syncthreads();
    }
    if (t == 0) kept[s] = carry;
    __syncthreads();
  }
}

template <bool HasPaste, bool HasSweeps>
__device__ __forceinline__ void write_block(const Args &a, const PasteArgs *pa, const SweepArgs *wa,
                                            const int *__restrict__ block_offs, const int *__restrict__ kept,
                                            float *__restrict__ out) {
  __shared__ float tile[kBlock * kMaxC];
  __shared__ float packed[kBlock * kMaxC];
  __shared__ int wsum[kWaves];
  __shared__ float planes[HasPaste ? kMaxBoxes * kPlaneFloats : 1];
  __shared__ uint32_t segs[HasSweeps ? kMaxSegments * kSegmentDwords : 1];
  const int si = sample_of_block(a, blockIdx.x);
  const Sample &sp = a.s[si];
  const int C = a.C;
  const long long first = (long long)(blockIdx.x - sp.block0) * kBlock;
  const int rows = sp.n - first < kBlock ? (int)(sp.n - first) : kBlock;
  if constexpr (HasPaste) {
    stage_rows_paste(pa->p[si], sp.src, first, rows, C, tile, planes);
  } else {
    stage_rows<kBlock>(sp.src, first, rows, C, tile);
  }
  if constexpr (HasSweeps) stage_segments(wa->w[si], segs);
  __syncthreads();
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  bool keep = false;
  float x = 0.f, y = 0.f, z = 0.f;
  if (t < rows) {
    x = tile[t * C], y = tile[t * C + 1], z = tile[t * C + 2];
    bool dropped = false;
    if constexpr (HasSweeps) {
      long long r = first + t;
      if constexpr (HasPaste) r -= pa->p[si].m;
      if (wa->w[si].nseg > 0 && r >= 0) {
        float dt;
        dropped = !sweep_row(segs, wa->w[si].nseg, r, x, y, z, dt);
        tile[t * C + 4] = dt;  // the thread's own row: it alone reads it back below (C >= 5: the entry checks)
      }
    }
    if constexpr (HasPaste) dropped = dropped || (first + t >= pa->p[si].m && inside_any_box(planes, pa->p[si].K, x, y, z));
    keep = transform(sp, x, y, z);
    if constexpr (HasPaste || HasSweeps) keep = keep && !dropped;
  }
  const unsigned long long bal = __ballot(keep);
  const int in_wave = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wv] = __popcll(bal);
  __syncthreads();
  int woff = 0, block_kept = 0;
  for (int k = 0; k < kWaves; ++k) {
    if (k < wv) woff += wsum[k];
    block_kept += wsum[k];
  }
  const int local = woff + in_wave;          // rank inside the block
  const int boff = block_offs[blockIdx.x];   // kept rows of the sample before this block
  if (sp.flags & kShuffle) {                 // block-uniform
    if (keep) {
      const uint32_t row = permute((uint32_t)(boff + local), (uint32_t)kept[si], sp.key);
      float *dst = out + ((size_t)sp.row0 + row) * C;
      dst[0] = x, dst[1] = y, dst[2] = z;
      for (int c = 3; c < C; ++c) dst[c] = tile[t * C + c];
    }
    return;
  }
  if (keep) {
    float *dst = packed + local * C;
    dst[0] = x, dst[1] = y, dst[2] = z;
    for (int c = 3; c < C; ++c) dst[c] = tile[t * C + c];
  }
  __syncthreads();
  float *dst = out + ((size_t)sp.row0 + boff) * C;
  const int nd = block_kept * C;
  for (int d = t; d < nd; d += kBlock) dst[d] = packed[d];
}

__global__ __launch_bounds__(kBlock) void points_write_kernel(Args a, const int *__restrict__ block_offs,
                                                              const int *__restrict__ kept, float *__restrict__ out) {
  write_block<false, false>(a, nullptr, nullptr, block_offs, kept, out);
}

__global__ __launch_bounds__(kBlock) void points_write_paste_kernel(Args a, PasteArgs pa, const int *__restrict__ block_offs,
                                                                    const int *__restrict__ kept, float *__restrict__ out) {
  write_block<true, false>(a, &pa, nullptr, block_offs, kept, out);
}

__global__ __launch_bounds__(kBlock) void points_write_sweeps_kernel(Args a, SweepArgs wa, const int *__restrict__ block_offs,
                                                                     const int *__restrict__ kept, float *__restrict__ out) {
  write_block<false, true>(a, nullptr, &wa, block_offs, kept, out);
}

__global__ __launch_bounds__(kBlock) void points_write_paste_sweeps_kernel(Args a, PasteArgs pa, SweepArgs wa,
                                                                           const int *__restrict__ block_offs,
                                                                           const int *__restrict__ kept, float *__restrict__ out) {
  write_block<true, true>(a, &pa, &wa, block_offs, kept, out);
}

long long blocks_of(long long n) { return (n + kBlock - 1) / kBlock; }

// the descriptor copy: a sample of `rows` rows (pasted ones included) from block `block0` of the launch and output row `row0`
void fill(Sample &d, const bfhip_points_aug_sample &s, int rows, int block0, int row0) {
  d.src = s.points;
  d.n = rows;
  d.block0 = block0;
  d.row0 = row0;
  d.flags = s.flags;
  for (int k = 0; k < 9; ++k) d.r[k] = s.rot[k];
  for (int k = 0; k < 3; ++k) d.t[k] = s.trans[k];
  d.s = s.scale;
  for (int k = 0; k < 6; ++k) d.range[k] = s.range[k];
  for (int k = 0; k < kRounds; ++k) d.key[k] = s.keys[k];
}

// the count and the write launch of a chunk: each kernel receives the argument structs of its variant and no others
void launch_count(bool paste, bool sweeps, unsigned blocks, hipStream_t st, const Args &a, const PasteArgs &pa,
                  const SweepArgs &wa, int *counts) {
  if (paste && sweeps)
    hipLaunchKernelGGL(points_count_paste_sweeps_kernel, dim3(blocks), dim3(kBlock), 0, st, a, pa, wa, counts);
  else if (paste)
    hipLaunchKernelGGL(points_count_paste_kernel, dim3(blocks), dim3(kBlock), 0, st, a, pa, counts);
  else if (sweeps)
    hipLaunchKernelGGL(points_count_sweeps_kernel, dim3(blocks), dim3(kBlock), 0, st, a, wa, counts);
  else
    hipLaunchKernelGGL(points_count_kernel, dim3(blocks), dim3(kBlock), 0, st, a, counts);
}

void launch_write(bool paste, bool sweeps, unsigned blocks, hipStream_t st, const Args &a, const PasteArgs &pa,
                  const SweepArgs &wa, const int *offs, const int *kept, float *out) {
  if (paste && sweeps)
    hipLaunchKernelGGL(points_write_paste_sweeps_kernel, dim3(blocks), dim3(kBlock), 0, st, a, pa, wa, offs, kept, out);
  else if (paste)
    hipLaunchKernelGGL(points_write_paste_kernel, dim3(blocks), dim3(kBlock), 0, st, a, pa, offs, kept, out);
  else if (sweeps)
    hipLaunchKernelGGL(points_write_sweeps_kernel, dim3(blocks), dim3(kBlock), 0, st, a, wa, offs, kept, out);
  else
    hipLaunchKernelGGL(points_write_kernel, dim3(blocks), dim3(kBlock), 0, st, a, offs, kept, out);
}

// The host side of the three entries, `what` the entry's name in its messages.  pastes / sweeps: one descriptor per sample, or
// NULL for the kernels without that variant (a given table selects its variant even when every descriptor in it is empty).
// Everything is checked before the first launch: a rejected call launches nothing.
int run_points_aug(const char *what, const bfhip_points_aug_sample *samples, const bfhip_points_aug_paste_desc *pastes,
                   const bfhip_points_aug_sweeps_desc *sweeps, int min_C, int n_samples, int C, float *out, int32_t *kept,
                   void *workspace, size_t workspace_bytes, void *stream) {
  BFHIP_REQUIRE(samples && kept, "%s: a required pointer is NULL", what);
  BFHIP_REQUIRE(n_samples >= 1, "%s: n_samples=%d", what, n_samples);
  BFHIP_REQUIRE(C >= min_C && C <= kMaxC, "%s: %d columns (%d .. %d%s)", what, C, min_C, kMaxC,
                sweeps ? ": column 4 takes the time lag" : "");
  long long total = 0;
  for (int i = 0; i < n_samples; ++i) {
    const bfhip_points_aug_sample &s = samples[i];
    BFHIP_REQUIRE(s.n >= 0 && (s.n == 0 || s.points), "%s: sample %d: n=%d points=%p", what, i, s.n, (const void *)s.points);
    BFHIP_REQUIRE((s.flags & ~63) == 0, "%s: sample %d: flags 0x%x", what, i, s.flags);
    BFHIP_REQUIRE(((uintptr_t)s.points & 3) == 0, "%s: sample %d: points not 4-byte aligned", what, i);
    total += s.n;
    if (sweeps) {
      const bfhip_points_aug_sweeps_desc &w = sweeps[i];
      BFHIP_REQUIRE(w.n_segments >= 0 && w.n_segments <= kMaxSegments && (w.n_segments == 0 || w.segments),
                    "%s: sample %d: n_segments=%d (0 .. %d) segments=%p", what, i, w.n_segments, kMaxSegments,
                    (const void *)w.segments);
      BFHIP_REQUIRE(((uintptr_t)w.segments & 7) == 0, "%s: sample %d: segments not 8-byte aligned", what, i);
      if (w.n_segments > 0) {
        BFHIP_REQUIRE(w.first[0] == 0 && w.first[w.n_segments] == s.n,
                      "%s: sample %d: boundaries run from %d to %d, the sample's rows from 0 to %d", what, i, w.first[0],
                      w.first[w.n_segments], s.n);
        for (int k = 0; k < w.n_segments; ++k)
          BFHIP_REQUIRE(w.first[k] <= w.first[k + 1], "%s: sample %d: boundary %d (%d) is below boundary %d (%d)", what, i, k + 1,
                        w.first[k + 1], k, w.first[k]);
      }
    }
    if (pastes) {
      const bfhip_points_aug_paste_desc &p = pastes[i];
      BFHIP_REQUIRE(p.n_points >= 0 && (p.n_points == 0 || p.points), "%s: sample %d: n_points=%d points=%p", what, i, p.n_points,
                    (const void *)p.points);
      BFHIP_REQUIRE(p.n_boxes >= 0 && p.n_boxes <= kMaxBoxes && (p.n_boxes == 0 || p.planes),
                    "%s: sample %d: n_boxes=%d (0 .. %d) planes=%p", what, i, p.n_boxes, kMaxBoxes, (const void *)p.planes);
      BFHIP_REQUIRE((((uintptr_t)p.points | (uintptr_t)p.planes) & 3) == 0, "%s: sample %d: a paste pointer is not 4-byte aligned",
                    what, i);
      total += p.n_points;
    }
  }
  BFHIP_REQUIRE(total <= 0x7fffffffll, "%s: %lld rows in all (below 2^31)", what, total);
  BFHIP_REQUIRE(total == 0 || out, "%s: out is NULL", what);
  const size_t need = bfhip_points_aug_workspace_bytes(total, n_samples);
  BFHIP_REQUIRE(workspace_bytes >= need && (workspace || total == 0), "%s: workspace of %zu bytes, %zu needed", what,
                workspace_bytes, need);
  const hipStream_t st = (hipStream_t)stream;
  auto launched = [what](const char *kernel) {
    char label[64];
    snprintf(label, sizeof(label), "%s %s", what, kernel);
    return check_launch(label);
  };
  int *counts = (int *)workspace;
  long long row0 = 0;
  for (int first = 0; first < n_samples; first += kMaxSamples) {
    const int n = n_samples - first < kMaxSamples ? n_samples - first : kMaxSamples;
    Args a;
    PasteArgs pa;
    SweepArgs wa;
    a.n_samples = n;
    a.C = C;
    long long blocks = 0;
    for (int i = 0; i < kMaxSamples; ++i) {
      // a slot i >= n is never reached by a block: the last real descriptor with no rows, block0 = the launch's block count
      const bool real = i < n;
      const int j = first + (real ? i : n - 1);
      pa.p[i] = real && pastes ? Paste{pastes[j].points, pastes[j].planes, pastes[j].n_points, pastes[j].n_boxes}
                               : Paste{nullptr, nullptr, 0, 0};
      wa.w[i] = real && sweeps ? Sweeps{sweeps[j].segments, sweeps[j].n_segments} : Sweeps{nullptr, 0};
      // the row space: pasted rows, then the sample's own (the keyframe and the sweeps)
      const long long rows = real ? (long long)samples[j].n + pa.p[i].m : 0;
      fill(a.s[i], samples[j], (int)rows, (int)blocks, (int)row0);
      blocks += blocks_of(rows);
      row0 += rows;
    }
    int rc;
    if (blocks > 0) {
      launch_count(pastes != nullptr, sweeps != nullptr, (unsigned)blocks, st, a, pa, wa, counts);
      if ((rc = launched("count")) != BFHIP_OK) return rc;
    }
    // always launched: an all-empty chunk still needs its kept counts (zero) written
    hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, a, (int)blocks, counts, kept + first);
    if ((rc = launched("scan")) != BFHIP_OK) return rc;
    if (blocks > 0) {
      launch_write(pastes != nullptr, sweeps != nullptr, (unsigned)blocks, st, a, pa, wa, counts, kept + first, out);
      if ((rc = launched("write")) != BFHIP_OK) return rc;
    }
    counts += blocks;
  }
  return BFHIP_OK;
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_points_aug_block(void) { return kBlock; }

BFHIP_EXPORT int bfhip_points_aug_max_boxes(void) { return kMaxBoxes; }

BFHIP_EXPORT int bfhip_points_aug_max_sweeps(void) { return kMaxSegments; }

BFHIP_EXPORT size_t bfhip_points_aug_workspace_bytes(long long total_rows, int n_samples) {
  if (total_rows < 0 || n_samples < 0) return 0;
  // one int per block; a sample's last block may be partial
  return align_up((size_t)(blocks_of(total_rows) + n_samples) * sizeof(int), 256);
}

BFHIP_EXPORT int bfhip_points_aug(const bfhip_points_aug_sample *samples_host, int n_samples, int C, float *out, int32_t *kept,
                                  void *workspace, size_t workspace_bytes, void *stream) {
  return run_points_aug("points_aug", samples_host, nullptr, nullptr, 3, n_samples, C, out, kept, workspace, workspace_bytes,
                        stream);
}

BFHIP_EXPORT int bfhip_points_aug_paste(const bfhip_points_aug_sample *samples_host,
                                        const bfhip_points_aug_paste_desc *pastes_host, int n_samples, int C, float *out,
                                        int32_t *kept, void *workspace, size_t workspace_bytes, void *stream) {
  BFHIP_REQUIRE(pastes_host, "points_aug_paste: a required pointer is NULL");
  return run_points_aug("points_aug_paste", samples_host, pastes_host, nullptr, 3, n_samples, C, out, kept, workspace,
                        workspace_bytes, stream);
}

// pastes_host may be NULL: the kernels without the paste
BFHIP_EXPORT int bfhip_points_aug_sweeps(const bfhip_points_aug_sample *samples_host,
                                         const bfhip_points_aug_paste_desc *pastes_host,
                                         const bfhip_points_aug_sweeps_desc *sweeps_host, int n_samples, int C, float *out,
                                         int32_t *kept, void *workspace, size_t workspace_bytes, void *stream) {
  BFHIP_REQUIRE(sweeps_host, "points_aug_sweeps: a required pointer is NULL");
  return run_points_aug("points_aug_sweeps", samples_host, pastes_host, sweeps_host, 5, n_samples, C, out, kept, workspace,
                        workspace_bytes, stream);
}

