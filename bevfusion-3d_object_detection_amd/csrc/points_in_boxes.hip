// points_in_boxes.hip -- which rows of a cloud lie in which rotated box, compacted box by box (gfx950): the hot loop of the
// ground-truth database builder, box_np_ops.points_in_rbbox + one gather per box (tools/dataset_converters/create_gt_database.py
// :257,296-297 of the reference), as box_ops.torch_points_in_boxes defines it.
//
// Membership: row i is in box j unless some plane k of the box has ((x n0 + y n1) + z n2) + d >= 0, every product and sum a
// separate float32 operation (__fmul_rn / __fadd_rn: nothing contracts them).  The test is "not (sign >= 0)": a NaN sign leaves
// the row inside, as the reference's loop does.  The planes are points_aug.paste_planes(boxes), made on the host.
//
// Three launches, count -> scan -> ranked write (points_aug.hip, voxelize.hip 2a-2c):
//   1. pib_count_kernel: one workgroup of kBlock threads per kBlock consecutive rows, staged through LDS with coalesced dword
//      reads (stage_rows of points_tile.h).  The plane table goes through LDS in chunks of kChunk = 64 boxes (24 floats per
//      box, 6 KB); all lanes of a wave read the same plane at the same time (an LDS broadcast) and leave a box at its first plane
//      with sign >= 0.  Per box one wave __ballot: its popcount is the wave's member count, its bit of the lane goes into the
//      lane's 64-bit membership word of the chunk.  Out: the words, member[n][W], W = ceil(K / 64), and the per (box, workgroup)
//      counts, block_counts[K][blocks].
//   2. pib_scan_kernel: one workgroup per box scans the box's row of block_counts (exclusive, in place: the rows of the box in
//      earlier workgroups) and writes counts[box].
//   3. pib_gather_kernel: the same row tiles; membership is READ BACK from the words, not recomputed (8 W bytes per row instead of
//      up to 6 K plane evaluations, and the two passes cannot disagree).  Every workgroup turns counts[K] into the boxes' first
//      rows (an exclusive scan of at most kMaxBoxes values in LDS, 64-bit).  A member's rank inside its workgroup = the members in
//      earlier waves (ballot popcounts through LDS) + the member lanes below it; row start[j] + block offset + rank of the output
//      gets the row, with the box's bottom centre subtracted from columns 0..2 when centres are given (one float32 subtraction
//      each).  A wave none of whose rows is in any box of a chunk -- most waves -- does nothing for that chunk.
// No atomics anywhere: every output is a pure function of the inputs, the same bytes on every run.  No launch waits on another
// block of the same launch.
#include "common.h"
#include "points_tile.h"

namespace bfhip {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxC = 8;
constexpr int kChunk = 64;         // boxes per LDS plane table and per membership word
constexpr int kMaxBoxes = 256;     // boxes per call: the gather scans counts[K] with one thread per box
static_assert(kChunk == kWave && kMaxBoxes <= kBlock, "one lane per box of a chunk, one thread per box of a call");

__global__ __launch_bounds__(kBlock) void pib_count_kernel(const float *__restrict__ points, int n, int C,
                                                           const float *__restrict__ planes_g, int K, int blocks,
                                                           int *__restrict__ block_counts,
                                                           unsigned long long *__restrict__ member) {
  __shared__ float tile[kBlock * kMaxC];
  __shared__ __align__(16) float planes[kChunk * kPlaneFloats];
  __shared__ int wcnt[kWaves][kChunk];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const long long first = (long long)blockIdx.x * kBlock;
  const int rows = n - first < kBlock ? (int)(n - first) : kBlock;
  const int W = (K + kChunk - 1) / kChunk;
  stage_rows<kBlock>(points, first, rows, C, tile);
  __syncthreads();
  float x = 0.f, y = 0.f, z = 0.f;
  const bool live = t < rows;
  if (live) x = tile[t * C], y = tile[t * C + 1], z = tile[t * C + 2];
  for (int c = 0; c < W; ++c) {
    const int kc = K - c * kChunk < kChunk ? K - c * kChunk : kChunk;
    const float *src = planes_g + (size_t)c * kChunk * kPlaneFloats;
    for (int d = t; d < kc * kPlaneFloats; d += kBlock) planes[d] = src[d];
    __syncthreads();
    unsigned long long word = 0ull;
    for (int j = 0; j < kc; ++j) {
      const float *pl = planes + j * kPlaneFloats;
      bool inside = live;
      if (inside) {
        for (int k = 0; k < 6; ++k) {
          if (plane_sign(pl + 4 * k, x, y, z) >= 0.f) {  // NaN: not left
            inside = false;
            break;
          }
        }
      }
      const unsigned long long bal = __ballot(inside);
      if (lane == 0) wcnt[wv][j] = __popcll(bal);
      if (inside) word |= 1ull << j;
    }
    if (live) member[(size_t)(first + t) * W + c] = word;
    __syncthreads();
    if (t < kc) {
      int tot = 0;
      for (int w = 0; w < kWaves; ++w) tot += wcnt[w][t];
      block_counts[(size_t)(c * kChunk + t) * blocks + blockIdx.x] = tot;
    }
    __syncthreads();  // planes and wcnt are rewritten by the next chunk
  }
}

// exclusive block scan of one value per thread (kBlock threads); *total = the sum.  wtot: kWaves values of LDS.
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *wtot, T *total) {
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  T incl = v;
  for (int o = 1; o < kWave; o <<= 1) {
    const T up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == kWave - 1) wtot[wv] = incl;
  __syncthreads();
  T woff = 0, all = 0;
  for (int k = 0; k < kWaves; ++k) {
    if (k < wv) woff += wtot[k];
    all += wtot[k];
  }
  *total = all;
  return woff + incl - v;
}

// box blockIdx.x: its row of block_counts becomes the exclusive prefix over the workgroups; counts[box] = the total.  Thread t
// owns a contiguous run of the row.
__global__ __launch_bounds__(kBlock) void pib_scan_kernel(int blocks, int *__restrict__ block_counts, int *__restrict__ counts) {
  __shared__ int wtot[kWaves];
  int *row = block_counts + (size_t)blockIdx.x * blocks;
  const int per = (blocks + kBlock - 1) / kBlock;
  const long long lo = (long long)threadIdx.x * per;
  const int b0 = lo < blocks ? (int)lo : blocks;
  const int b1 = lo + per < blocks ? (int)(lo + per) : blocks;
  int sum = 0;
  for (int i = b0; i < b1; ++i) sum += row[i];
  int total;
  int run = block_exclusive_scan<int>(sum, wtot, &total);
  for (int i = b0; i < b1; ++i) {
    const int v = row[i];
    row[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void pib_gather_kernel(const float *__restrict__ points, int n, int C,
                                                            const float *__restrict__ centers, int K, int blocks,
                                                            const int *__restrict__ block_offs, const int *__restrict__ counts,
                                                            const unsigned long long *__restrict__ member,
                                                            float *__restrict__ out, long long capacity) {
  __shared__ float tile[kBlock * kMaxC];
  __shared__ long long base[kMaxBoxes];   // first output row of (box, this workgroup)
  __shared__ float ctr[kMaxBoxes * 3];
  __shared__ long long wtot[kWaves];
  __shared__ int wcnt[kWaves][kChunk];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const long long first = (long long)blockIdx.x * kBlock;
  const int rows = n - first < kBlock ? (int)(n - first) : kBlock;
  const int W = (K + kChunk - 1) / kChunk;
  stage_rows<kBlock>(points, first, rows, C, tile);
  long long total;
  const long long start = block_exclusive_scan<long long>(t < K ? (long long)counts[t] : 0ll, wtot, &total);
  if (t < K) base[t] = start + block_offs[(size_t)t * blocks + blockIdx.x];
  if (centers)
    for (int d = t; d < K * 3; d += kBlock) ctr[d] = centers[d];
  __syncthreads();
  const bool live = t < rows;
  for (int c = 0; c < W; ++c) {
    const int kc = K - c * kChunk < kChunk ? K - c * kChunk : kChunk;
    const unsigned long long word = live ? member[(size_t)(first + t) * W + c] : 0ull;
    const bool wave_has = __ballot(word != 0ull) != 0ull;  // wave-uniform
    if (wave_has) {
      for (int j = 0; j < kc; ++j) {
        const unsigned long long bal = __ballot((word >> j) & 1ull);
        if (lane == 0) wcnt[wv][j] = __popcll(bal);
      }
    } else if (lane < kc) {
      wcnt[wv][lane] = 0;
    }
    __syncthreads();
    if (wave_has) {
      for (int j = 0; j < kc; ++j) {
        const bool in = (word >> j) & 1ull;
        const unsigned long long bal = __ballot(in);
        if (bal == 0ull) continue;
        if (in) {
          int rank = __popcll(bal & ((1ull << lane) - 1ull));
          for (int w = 0; w < wv; ++w) rank += wcnt[w][j];
          const int box = c * kChunk + j;
          const long long row = base[box] + rank;
          if (row < capacity) {  // holds whenever capacity >= the total the entry was given; never writes past `out`
            float *dst = out + (size_t)row * C;
            const float *srcrow = tile + t * C;
            if (centers) {
              dst[0] = __fsub_rn(srcrow[0], ctr[box * 3]);
              dst[1] = __fsub_rn(srcrow[1], ctr[box * 3 + 1]);
              dst[2] = __fsub_rn(srcrow[2], ctr[box * 3 + 2]);
            } else {
              dst[0] = srcrow[0], dst[1] = srcrow[1], dst[2] = srcrow[2];
            }
            for (int k = 3; k < C; ++k) dst[k] = srcrow[k];
          }
        }
      }
    }
    __syncthreads();  // wcnt is rewritten by the next chunk
  }
}

long long blocks_of(long long n) { return (n + kBlock - 1) / kBlock; }
size_t offsets_bytes(long long n, int K) { return align_up((size_t)blocks_of(n) * (size_t)K * sizeof(int), 256); }
size_t member_bytes(long long n, int K) {
  return align_up((size_t)n * (size_t)((K + kChunk - 1) / kChunk) * sizeof(unsigned long long), 256);
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_points_in_boxes_block(void) { return kBlock; }

BFHIP_EXPORT int bfhip_points_in_boxes_max_boxes(void) { return kMaxBoxes; }

BFHIP_EXPORT size_t bfhip_points_in_boxes_workspace_bytes(long long n, int K) {
  if (n < 0 || n > 0x7fffffffll || K < 0 || K > kMaxBoxes) return 0;
  return offsets_bytes(n, K) + member_bytes(n, K);
}

BFHIP_EXPORT int bfhip_points_in_boxes_count(const float *points, long long n, int C, const float *planes, int K, int32_t *counts,
                                             uint64_t *member, void *workspace, size_t workspace_bytes, void *stream) {
  BFHIP_REQUIRE(n >= 0 && n < 0x80000000ll, "points_in_boxes_count: n=%lld (0 .. 2^31 - 1)", n);
  BFHIP_REQUIRE(C >= 3 && C <= kMaxC, "points_in_boxes_count: %d columns (3 .. %d)", C, kMaxC);
  BFHIP_REQUIRE(K >= 0 && K <= kMaxBoxes, "points_in_boxes_count: K=%d boxes (0 .. %d)", K, kMaxBoxes);
  BFHIP_REQUIRE(n == 0 || points, "points_in_boxes_count: points is NULL with n=%lld", n);
  BFHIP_REQUIRE(K == 0 || (planes && counts), "points_in_boxes_count: planes or counts is NULL with K=%d", K);
  BFHIP_REQUIRE((((uintptr_t)points | (uintptr_t)planes | (uintptr_t)counts) & 3) == 0,
                "points_in_boxes_count: points, planes or counts not 4-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)member & 7) == 0, "points_in_boxes_count: member not 8-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)workspace & 255) == 0, "points_in_boxes_count: workspace not 256-byte aligned");
  const size_t need = bfhip_points_in_boxes_workspace_bytes(n, K);
  BFHIP_REQUIRE(workspace_bytes >= need && (workspace || need == 0), "points_in_boxes_count: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  if (K == 0) return BFHIP_OK;  // nothing to write
  const int blocks = (int)blocks_of(n);
  int *block_counts = (int *)workspace;
  unsigned long long *words = member ? (unsigned long long *)member : (unsigned long long *)((char *)workspace + offsets_bytes(n, K));
  if (blocks > 0) {
    hipLaunchKernelGGL(pib_count_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, points, (int)n, C, planes, K,
                       blocks, block_counts, words);
    const int rc = check_launch("points_in_boxes count");
    if (rc != BFHIP_OK) return rc;
  }
  // always launched: with no rows the counts (zero) are still written
  hipLaunchKernelGGL(pib_scan_kernel, dim3((unsigned)K), dim3(kBlock), 0, (hipStream_t)stream, blocks, block_counts, counts);
  return check_launch("points_in_boxes scan");
}

BFHIP_EXPORT int bfhip_points_in_boxes_gather(const float *points, long long n, int C, const float *centers, int K,
                                              const int32_t *counts, const uint64_t *member, long long total, float *out,
                                              long long capacity, const void *workspace, size_t workspace_bytes, void *stream) {
  BFHIP_REQUIRE(n >= 0 && n < 0x80000000ll, "points_in_boxes_gather: n=%lld (0 .. 2^31 - 1)", n);
  BFHIP_REQUIRE(C >= 3 && C <= kMaxC, "points_in_boxes_gather: %d columns (3 .. %d)", C, kMaxC);
  BFHIP_REQUIRE(K >= 0 && K <= kMaxBoxes, "points_in_boxes_gather: K=%d boxes (0 .. %d)", K, kMaxBoxes);
  BFHIP_REQUIRE(total >= 0 && total < 0x80000000ll, "points_in_boxes_gather: %lld member rows in all (0 .. 2^31 - 1)", total);
  BFHIP_REQUIRE(capacity >= total, "points_in_boxes_gather: out holds %lld rows, %lld needed", capacity, total);
  BFHIP_REQUIRE(n == 0 || points, "points_in_boxes_gather: points is NULL with n=%lld", n);
  BFHIP_REQUIRE(K == 0 || counts, "points_in_boxes_gather: counts is NULL with K=%d", K);
  BFHIP_REQUIRE(total == 0 || out, "points_in_boxes_gather: out is NULL with %lld rows to write", total);
  BFHIP_REQUIRE((((uintptr_t)points | (uintptr_t)centers | (uintptr_t)counts | (uintptr_t)out) & 3) == 0,
                "points_in_boxes_gather: points, centers, counts or out not 4-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)member & 7) == 0, "points_in_boxes_gather: member not 8-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)workspace & 255) == 0, "points_in_boxes_gather: workspace not 256-byte aligned");
  const size_t need = bfhip_points_in_boxes_workspace_bytes(n, K);
  BFHIP_REQUIRE(workspace_bytes >= need && (workspace || need == 0), "points_in_boxes_gather: workspace of %zu bytes, %zu needed",
                workspace_bytes, need);
  const int blocks = (int)blocks_of(n);
  if (K == 0 || blocks == 0 || total == 0) return BFHIP_OK;
  const int *block_offs = (const int *)workspace;
  const unsigned long long *words =
      member ? (const unsigned long long *)member : (const unsigned long long *)((const char *)workspace + offsets_bytes(n, K));
  hipLaunchKernelGGL(pib_gather_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, points, (int)n, C, centers, K,
                     blocks, block_offs, counts, words, out, capacity);
  return check_launch("points_in_boxes gather");
}
