// spconv.hip -- sparse 3-D convolution (SubMConv3d / SparseConv3d, traveller59 layout) for gfx950: the forward / data-gradient
// gather-GEMMs.  The rulebooks are in spconv_rulebook.hip, the weight gradient in spconv_wgrad.hip (fp32 MFMA) and
// spconv_wgrad_tr.hip (bf16 MFMA), the sparse <-> BEV scatters in sparse_bev.hip; spconv_common.h is what they share.
//
// Replaces what the reference delegates to the third-party spconv 2.x wheel
// (call sites: BF/sparse_encoder.py:133-147, mmdet3d/models/layers/sparse_block.py:190-217;
//  shim: projects/SparseConvolution/sparse_functional.py:118-137 get_indice_pairs_implicit_gemm,
//  :287-314 implicit_gemm).  Layout conventions kept: indices i32[N,4] = (b, x, y, z);
//  pair_fwd i32[KV, N_out] with -1 holes (sparse_functional.py:57-61); weights (out, k0, k1, k2, in)
//  (mmdet3d/models/layers/spconv/overwrite_spconv/write_spconv2.py:50-51); kernel offset index
//  k = (i*k1 + j)*k2 + l.
//
// Rulebook:  SubM   -> open-addressing hash (linear cell -> row) + one lookup per (row, offset)
//            strided-> bitmap over the output grid + prefix popcount = output rows in ascending
//                      linear order (canonical, deterministic; spconv's order is hash-dependent)
// Compute :  output-stationary implicit GEMM on the MFMA units (exact fp32: v_mfma_f32_16x16x4_f32; bf16 inputs with fp32
//            accumulate: v_mfma_f32_16x16x32_bf16).  A workgroup of 4 waves owns 4*R*16 output rows x all C_out columns:
//            each wave accumulates its own R*16 rows, the 4 waves share every pre-packed weight tile through LDS (double
//            buffered, one barrier per (offset, channel chunk) step).  The workgroup loops over the KV offsets and skips
//            those none of its rows has, a wave skips the MFMAs of those none of ITS rows has; A rows are gathered
//            straight from L2 with 16-byte loads per lane (K permuted consistently in the packed weights, so no
//            shuffle), no atomics -> deterministic.  The same kernels compute dgrad (weights transposed, pair_bwd).
//            The pieces every variant shares (row ownership, offset masks, operand policy, epilogue) are written once
//            below; a variant is its load pipeline (the two-ahead one with its own weight-tile and MFMA text, see there).
#include "spconv_common.h"

namespace bfhip {
namespace {

// -------------------------------------------------------------------------------- weight packing
// Wp[((k*CC + cc)*NT + nt)*64 + lane][j] = T(M_k[(cc*4 + (lane>>4))*KPL + j][nt*16 + (lane&15)]),  j < KPL
//   KPL = K elements per lane and step: (float, 4) for the 16x16x4 fp32 MFMA, 16 channels per chunk cc;
//                                       (__bf16, 8) for the 16x16x32 bf16 MFMA, 32 channels per chunk
//   forward : M_k[ci][co] = W[co][k][ci]                      (K = C_in,  N = C_out)
//   dgrad   : M_k[co][ci] = W[co][flip ? KV-1-k : k][ci]      (K = C_out, N = C_in)
template <typename T, int KPL>
__global__ __launch_bounds__(256) void pack_weights_kernel(const float *__restrict__ W, int Cout, int KV, int Cin,
                                                           int transpose, int flip, int CC, int NT, T *__restrict__ Wp) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)KV * CC * NT * 64 * KPL;
  if (t >= total) return;
  int j = (int)(t % KPL);
  int lane = (int)((t / KPL) & 63);
  long long r = t / (64 * KPL);
  int nt = (int)(r % NT); r /= NT;
  int cc = (int)(r % CC);
  int k = (int)(r / CC);
  int kk = (cc * 4 + (lane >> 4)) * KPL + j;  // K index
  int nn = nt * 16 + (lane & 15);             // N index
  float v = 0.f;
  if (!transpose) {
    if (kk < Cin && nn < Cout) v = W[((size_t)nn * KV + k) * Cin + kk];
  } else {
    int ks = flip ? KV - 1 - k : k;
    if (kk < Cout && nn < Cin) v = W[((size_t)kk * KV + ks) * Cin + nn];
  }
  Wp[t] = (T)v;
}

// -------------------------------------------------------------------------------- shared pieces of the gather-GEMMs
// Lane geometry everywhere below: lane = tid & 63, wave wv = tid >> 6, lr = lane & 15 (row of a 16-row tile as A operand,
// column as C/D), lq = lane >> 4 (K quarter as operand, row quarter as C/D).

// Rows of this wave: position in (mask-sorted) order -> actual output row, -1 past the end.  Lane (lr, *) holds row r*16 + lr.
template <int R>
__device__ __forceinline__ void wave_rows(int n_rows, const int *__restrict__ perm, int (&my_row)[R]) {
  // XCD-chunked block order (common.h): each XCD walks one contiguous eighth of the (region-major sorted) rows
  const long long row_base = (xcd_chunked_block(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6)) * (R * 16);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    long long sp = row_base + r * 16 + (threadIdx.x & 15);
    my_row[r] = sp < n_rows ? (perm ? perm[sp] : (int)sp) : -1;
  }
}

// Which offsets this wave (wmask) and this workgroup (gmask) need: bit k = some row has a partner at offset k.  From the
// rulebook's row masks when it has them, else by asking probe(k, r) -- "row r of this lane has a partner at offset k" --
// for every offset.  Called by all threads of the workgroup: s_mask is zeroed and combined between two barriers here.
struct OffsetMasks { unsigned wmask, gmask; };
template <int R, typename Probe>
__device__ __forceinline__ OffsetMasks offset_masks(const unsigned *__restrict__ row_mask, const int (&my_row)[R], int KV,
                                                    Probe probe, unsigned *s_mask) {
  if (threadIdx.x == 0) *s_mask = 0u;
  __syncthreads();
  unsigned wmask = 0u;
  if (row_mask) {
    unsigned mm = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) mm |= my_row[r] >= 0 ? row_mask[my_row[r]] : 0u;
    for (int o = 32; o > 0; o >>= 1) mm |= __shfl_xor(mm, o);
    wmask = mm;
  } else {
    for (int k = 0; k < KV; ++k) {
      bool any = false;
#pragma unroll
      for (int r = 0; r < R; ++r) any |= probe(k, r);
      if (__any(any)) wmask |= 1u << k;
    }
  }
  if ((threadIdx.x & 63) == 0 && wmask) atomicOr(s_mask, wmask);
  __syncthreads();
  return {wmask, *s_mask};
}

// first offset the workgroup needs (KV if none), and the next one after kk
__device__ __forceinline__ int first_offset(unsigned gmask, int KV) { return gmask ? __ffs(gmask) - 1 : KV; }
__device__ __forceinline__ int next_offset(unsigned gmask, int kk, int KV) {
  return first_offset(gmask & ~((2u << kk) - 1u), KV);
}

// One packed weight tile (NT * 64 vectors) on its way global -> registers -> LDS, spread over the 256 threads: the one-ahead
// kernel's.  (The two-ahead kernel writes its own out: its load must be unconditional, see there, while here the threads
// past the tile issue none -- with NT = 1 or 2 that is most of the workgroup.)
template <typename V, int NT>
struct WeightTile {
  static constexpr int LOADS = (NT * 64 + 255) / 256;  // vectors per thread
  V pre[LOADS];
  __device__ __forceinline__ void load(const V *__restrict__ Wp, int k, int cc, int CC) {
    const V *wp = Wp + ((size_t)(k * CC + cc) * NT) * 64;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      int e = (int)threadIdx.x + i * 256;
      if (e < NT * 64) pre[i] = wp[e];
    }
  }
  __device__ __forceinline__ void stash(V *sB) const {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      int e = (int)threadIdx.x + i * 256;
      if (e < NT * 64) sB[e] = pre[i];
    }
  }
};

// Epilogue.  C/D layout: col = lane&15, row = (lane>>4)*4 + i ; the actual output row lives in lane (lq*4+i) of my_row.
// IO16: the output is rounded to bf16 once, here.
template <int NT, int R, bool IO16>
__device__ __forceinline__ void store_rows(const f32x4 (&acc)[R][NT], const int (&my_row)[R], int Ndim, void *__restrict__ out) {
  const int lr = threadIdx.x & 15, lq = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = __shfl(my_row[r], lq * 4 + i);
      if (row >= 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          int col = nt * 16 + lr;
          if (col < Ndim) {
            if (IO16) ((__bf16 *)out)[(size_t)row * Ndim + col] = (__bf16)acc[r][nt][i];
            else ((float *)out)[(size_t)row * Ndim + col] = acc[r][nt][i];
          }
        }
      }
    }
}

// ---- operand policies: what a lane loads of a gathered row per step (Raw), what the MFMA takes (Operand), the packed weight
// vector (Tile), CH channels per step of which a lane holds KPL consecutive ones from lq * KPL on, and mma(): the MFMAs of one
// step over the wave's R x NT output tiles, with the weight tile read from LDS.
// Exact fp32, v_mfma_f32_16x16x4_f32: lane l supplies A[row = l&15][k = l>>4], so the lane's four channels feed four MFMAs.
struct OpF32 {
  typedef f32x4 Tile, Raw, Operand;
  static constexpr int CH = 16, KPL = 4;
  static constexpr bool IO16 = false;
  static __device__ __forceinline__ Raw load(const void *__restrict__ in, size_t e) { return *(const f32x4 *)((const float *)in + e); }
  static __device__ __forceinline__ Operand to_operand(const Raw &a) { return a; }
  // the MFMAs of one step: four per tile, the lane's j-th channel against every tile before the (j+1)-th, so that MFMAs issued
  // back to back never wait for each other's accumulator (one tile's four in a row: 128 -> 128 at 6 000 rows 229 -> 247 us)
  template <int NT, int R>
  static __device__ __forceinline__ void mma(const Operand (&a)[R], const Tile *sB, f32x4 (&acc)[R][NT]) {
    f32x4 b[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b[nt] = sB[nt * 64 + (int)(threadIdx.x & 63)];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][j], b[nt][j], acc[r][nt], 0, 0, 0);
  }
};

// bf16 inputs, fp32 accumulate (the bf16 configs).  v_mfma_f32_16x16x32_bf16: lane l supplies A[row = l&15][k = 8*(l>>4) + j],
// B[k = 8*(l>>4) + j][col = l&15], j < 8, so one step covers 32 input channels with ONE MFMA per tile.
// IO16: features stored in bf16 (gathered rows are the MFMA operand as they are: one 16-byte load per lane and step, half the
// gather traffic of fp32 storage) and the output rounded to bf16 once; otherwise fp32 in HBM (two float4 gathers per lane and
// row tile, converted when consumed) and fp32 out.
struct F32Pair { f32x4 lo, hi; };
template <bool IO16_>
struct OpBf16 {
  typedef bf16x8 Tile, Operand;
  typedef std::conditional_t<IO16_, f32x4, F32Pair> Raw;  // IO16: 8 bf16 carried in one 16-byte register group
  static constexpr int CH = 32, KPL = 8;
  static constexpr bool IO16 = IO16_;
  static __device__ __forceinline__ Raw load(const void *__restrict__ in, size_t e) {
    if constexpr (IO16) {
      return *(const f32x4 *)((const __bf16 *)in + e);
    } else {
      const float *src = (const float *)in + e;
      return {*(const f32x4 *)src, *(const f32x4 *)(src + 4)};
    }
  }
  static __device__ __forceinline__ Operand to_operand(const Raw &a) {
    if constexpr (IO16) {
      return __builtin_bit_cast(bf16x8, a);
    } else {
      bf16x8 o;
      o[0] = (__bf16)a.lo[0]; o[1] = (__bf16)a.lo[1]; o[2] = (__bf16)a.lo[2]; o[3] = (__bf16)a.lo[3];
      o[4] = (__bf16)a.hi[0]; o[5] = (__bf16)a.hi[1]; o[6] = (__bf16)a.hi[2]; o[7] = (__bf16)a.hi[3];
      return o;
    }
  }
  static __device__ __forceinline__ f32x4 mfma(const Operand &a, const Tile &b, f32x4 acc) {  // one tile, one step
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
  template <int NT, int R>
  static __device__ __forceinline__ void mma(const Operand (&a)[R], const Tile *sB, f32x4 (&acc)[R][NT]) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const bf16x8 b = sB[nt * 64 + (int)(threadIdx.x & 63)];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r][nt] = mfma(a[r], b, acc[r][nt]);
    }
  }
};

// -------------------------------------------------------------------------------- forward / dgrad
// One-ahead kernel: 4 waves share every weight tile through LDS (double buffered, one barrier per (offset, Op::CH-channel
// chunk) step); the workgroup skips offsets none of its 4*R*16 rows uses.  Weight traffic from L2 drops 4x versus one weight
// fetch per wave; A rows are still gathered per wave.
template <typename Op, int NT, int R>
__global__ __launch_bounds__(256) void spconv_gemm_kernel(const void *__restrict__ in, int Kdim,
                                                          const typename Op::Tile *__restrict__ Wp,
                                                          const int *__restrict__ pairs, int ld, int KV, int n_rows,
                                                          int Ndim, const int *__restrict__ perm,
                                                          const unsigned *__restrict__ row_mask, void *__restrict__ out) {
  __shared__ typename Op::Tile sB[2][NT * 64];
  __shared__ unsigned s_mask;
  const int lq = (threadIdx.x & 63) >> 4;
  const int CC = (Kdim + Op::CH - 1) / Op::CH;
  int my_row[R];
  wave_rows<R>(n_rows, perm, my_row);
  const OffsetMasks m = offset_masks<R>(
      row_mask, my_row, KV, [&](int k, int r) { return my_row[r] >= 0 && pairs[(size_t)k * ld + my_row[r]] >= 0; }, &s_mask);
  const unsigned wmask = m.wmask, gmask = m.gmask;

  f32x4 acc[R][NT];  // element by element: with `= {}` the 32 -> 32 layer (bf16 storage) measured 38.2 -> 39.1 us
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  WeightTile<typename Op::Tile, NT> wt;
  auto load_idx = [&](int kk, int *dst) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      dst[r] = (kk < KV && my_row[r] >= 0 && ((wmask >> kk) & 1u)) ? pairs[(size_t)kk * ld + my_row[r]] : -1;
  };
  auto gather = [&](const int *ix, int c, typename Op::Raw *dst) {
    const int ch = c * Op::CH + lq * Op::KPL;
#pragma unroll
    for (int r = 0; r < R; ++r)
      dst[r] = (ix[r] >= 0 && ch < Kdim) ? Op::load(in, (size_t)ix[r] * Kdim + ch) : typename Op::Raw{};
  };
  // software pipeline: weight tile i+1 (global->regs->LDS), A rows of step i+1 and the pair indices of
  // the NEXT offset are all in flight while the MFMAs of step i run
  int k = first_offset(gmask, KV);
  int cc = 0, buf = 0;
  int idx[R], idx_nxt[R];
  typename Op::Raw a[R], a_nxt[R];
  if (k < KV) {
    wt.load(Wp, k, 0, CC);
    load_idx(k, idx);
    load_idx(next_offset(gmask, k, KV), idx_nxt);
    gather(idx, 0, a);
  }
  while (k < KV) {
    wt.stash(sB[buf]);
    __syncthreads();
    int nk = k, ncc = cc + 1;
    if (ncc == CC) { ncc = 0; nk = next_offset(gmask, k, KV); }
    if (nk < KV) {
      wt.load(Wp, nk, ncc, CC);
      gather(ncc == 0 ? idx_nxt : idx, ncc, a_nxt);
    }
    if ((wmask >> k) & 1u) {
      typename Op::Operand op[R];
#pragma unroll
      for (int r = 0; r < R; ++r) op[r] = Op::to_operand(a[r]);
      Op::template mma<NT, R>(op, sB[buf], acc);
    }
    if (ncc == 0 && nk < KV) {  // moving on to offset nk: rotate the index registers, fetch the one after
#pragma unroll
      for (int r = 0; r < R; ++r) idx[r] = idx_nxt[r];
      load_idx(next_offset(gmask, nk, KV), idx_nxt);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = a_nxt[r];
    k = nk;
    cc = ncc;
    buf ^= 1;
  }
  store_rows<NT, R, Op::IO16>(acc, my_row, Ndim, out);
}

// generic fallback (any channel counts): one thread per (row, out channel); fp32 FMA-free sums
__global__ __launch_bounds__(256) void spconv_scalar_kernel(const float *__restrict__ in, int Kdim,
                                                            const float *__restrict__ W, int Cout_w,
                                                            int Cin_w, int transpose, int flip,
                                                            const int *__restrict__ pairs, int ld,
                                                            int KV, int n_rows, int Ndim,
                                                            float *__restrict__ out) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long row = t / Ndim;
  int col = (int)(t - row * Ndim);
  if (row >= n_rows) return;
  float acc = 0.f;
  for (int k = 0; k < KV; ++k) {
    int idx = pairs[(size_t)k * ld + row];
    if (idx < 0) continue;
    const float *x = in + (size_t)idx * Kdim;
    if (!transpose) {
      const float *w = W + ((size_t)col * KV + k) * Cin_w;  // W[co=col][k][ci]
      for (int c = 0; c < Kdim; ++c) acc = fmaf(x[c], w[c], acc);
    } else {
      int ks = flip ? KV - 1 - k : k;
      for (int c = 0; c < Kdim; ++c) acc = fmaf(x[c], W[((size_t)c * KV + ks) * Cin_w + col], acc);  // W[co=c][ks][ci=col]
    }
  }
  out[(size_t)row * Ndim + col] = acc;
}

// Two-ahead variant of spconv_gemm_kernel<OpBf16>: the same tiling (workgroup = 4 waves x R x 16 output rows, all NT column
// tiles, one (offset, 32-channel chunk) per step with the weight tile shared through LDS), restructured around latency.
// The one-ahead kernel issues the gathers and the weight-tile loads of step s+1 during step s: one step is only NT * R MFMAs
// (0.1-0.4 us), so most of every ~1 us round trip is exposed, 27 * CC times per workgroup.  Here
//  * all pair-table entries of the workgroup's rows are fetched once, back to back, into LDS (s_idx) -- no dependent
//    index load remains inside the loop;
//  * loads run TWO steps ahead: three register sets used cyclically (the loop is unrolled by 3 so that no set is copied
//    while its loads are in flight), gathers are unconditional from clamped addresses and masked when consumed.
// Row ownership, offset masks, operand loads / conversion and the epilogue are the shared helpers.  The loop keeps its own text
// for the weight tile, the next offset, the accumulator zeroing and the MFMAs: each was tried on the helper (WeightTile,
// next_offset, Op::mma) and timed against this form, same bits every time: 64 -> 64, 64 -> 128 and 128 -> 128 with bf16 storage
// came out 0.5-1.0 us slower with any of them (numbers in DESIGN.md); Op::mma and a zeroing helper also cost up to four
// instantiations 4 VGPRs and a wave of occupancy.  The generated loops are the same instructions in another order.
template <int NT, int R, bool IO16>
__global__ __launch_bounds__(256) void spconv_gemm_bf16p_kernel(const void *__restrict__ in_, int Kdim,
                                                                const bf16x8 *__restrict__ Wp,
                                                                const int *__restrict__ pairs, int ld,
                                                                int KV, int n_rows, int Ndim,
                                                                const int *__restrict__ perm,
                                                                const unsigned *__restrict__ row_mask,
                                                                void *__restrict__ out_) {
  typedef OpBf16<IO16> Op;
  __shared__ bf16x8 sB[2][NT * 64];
  __shared__ unsigned s_mask;
  __shared__ int s_idx[4][32][16 * R];  // [wave][offset][row of the wave]; KV <= 32 (checked by the host)
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int CC = (Kdim + 31) >> 5;
  int my_row[R];
  wave_rows<R>(n_rows, perm, my_row);
  // pair entries of this wave's rows for every offset: lane (lr, lq) takes offsets lq, lq + 4, ...
  {
    int v[8][R];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int kk = min(lq + 4 * j, KV - 1);
        v[j][r] = pairs[(size_t)kk * ld + max(my_row[r], 0)];
      }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (lq + 4 * j < KV) s_idx[wv][lq + 4 * j][r * 16 + lr] = my_row[r] >= 0 ? v[j][r] : -1;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const OffsetMasks m =
      offset_masks<R>(row_mask, my_row, KV, [&](int k, int r) { return s_idx[wv][k][r * 16 + lr] >= 0; }, &s_mask);
  const unsigned wmask = m.wmask, gmask = m.gmask;

  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int LOADS = (NT * 64 + 255) / 256;  // weight-tile vectors per thread
  struct Set {  // what one step needs from memory
    bf16x8 pre[LOADS];
    typename Op::Raw a[R];
    int ix[R];
  };
  auto next_set = [&](int kk) {
    unsigned rest = gmask & ~((2u << kk) - 1u);
    return rest ? __ffs(rest) - 1 : KV;
  };
  auto advance = [&](int &k, int &cc) {
    if (++cc == CC) { cc = 0; k = next_set(k); }
  };
  auto issue = [&](Set &st, int k, int cc) {  // weight tile of (k, cc) and the gathered operand rows; no waits
    const bf16x8 *wp = Wp + ((size_t)(k * CC + cc) * NT) * 64;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int e = tid + i * 256;
      st.pre[i] = wp[e < NT * 64 ? e : 0];  // unconditional: a load under a branch leaves the count of loads in flight
                                            // unknown, and every wait behind it becomes a wait for all (12-15 % slower)
    }
    const int ch = cc * 32 + lq * 8;
    const int chc = ch < Kdim ? ch : 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int ix = s_idx[wv][k][r * 16 + lr];
      st.ix[r] = ch < Kdim ? ix : -1;
      st.a[r] = Op::load(in_, (size_t)max(ix, 0) * Kdim + chc);
    }
  };
  int buf = 0;
  auto step = [&](Set &cur, Set &dst, int k, int k2, int cc2) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int e = tid + i * 256;
      if (e < NT * 64) sB[buf][e] = cur.pre[i];
    }
    __syncthreads();
    if (k2 < KV) issue(dst, k2, cc2);  // block-uniform: two steps ahead
    if ((wmask >> k) & 1u) {
      bf16x8 a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) a[r] = Op::to_operand(cur.ix[r] >= 0 ? cur.a[r] : typename Op::Raw{});
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf16x8 b = sB[buf][nt * 64 + lane];
#pragma unroll
        for (int r = 0; r < R; ++r)
          acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[r], b, acc[r][nt], 0, 0, 0);
      }
    }
    buf ^= 1;
  };
  Set s0, s1, s2;
  int k0 = gmask ? __ffs(gmask) - 1 : KV, c0 = 0;
  int k1 = k0, c1 = c0;
  if (k0 < KV) { issue(s0, k0, c0); advance(k1, c1); }
  int k2 = k1, c2 = c1;
  if (k1 < KV) { issue(s1, k1, c1); advance(k2, c2); }
  while (k0 < KV) {  // k0 / k1 / k2: offsets of the current step and the two after it (KV = none)
    step(s0, s2, k0, k2, c2);
    k0 = k1; c0 = c1; k1 = k2; c1 = c2; if (k2 < KV) advance(k2, c2);
    if (k0 >= KV) break;
    step(s1, s0, k0, k2, c2);
    k0 = k1; c0 = c1; k1 = k2; c1 = c2; if (k2 < KV) advance(k2, c2);
    if (k0 >= KV) break;
    step(s2, s1, k0, k2, c2);
    k0 = k1; c0 = c1; k1 = k2; c1 = c2; if (k2 < KV) advance(k2, c2);
  }
  store_rows<NT, R, IO16>(acc, my_row, Ndim, out_);
}

// -------------------------------------------------------------------------------- host side of both entry points
// bf16 = 0: exact fp32 MFMA; shapes the MFMA path does not take fall back to the scalar kernel.  bf16 = 1: bf16 MFMA inputs,
// io16 = features and output stored in bf16; other shapes are rejected.  `name` is the entry point's, for the messages.
// Kernel instantiations: NT in {1, 2, 4, 8} column tiles, R in {1, 2, 4} row tiles per wave; one workgroup = 4 waves x R*16 rows.
int spconv_gemm_impl(bool bf16, const char *name, const void *in, const float *W, const int32_t *pairs, int ld, int KV,
                     int n_rows, int Cin, int Cout, int transpose, int flip, const int32_t *perm, const uint32_t *row_mask,
                     void *out, bool io16, void *workspace, size_t workspace_bytes, hipStream_t stream) {
  BFHIP_REQUIRE(KV > 0 && (!bf16 || KV <= 32) && Cin > 0 && Cout > 0 && n_rows >= 0 && ld >= n_rows, "%s: bad sizes", name);
  if (n_rows == 0) return BFHIP_OK;
  BFHIP_REQUIRE(in && W && pairs && out, "%s: null pointer", name);
  const int Kdim = transpose ? Cout : Cin, Ndim = transpose ? Cin : Cout;
  const int KPL = bf16 ? OpBf16<false>::KPL : OpF32::KPL, CH = 4 * KPL;  // K elements per lane, channels per step
  const int NT = (Ndim + 15) / 16, CC = (Kdim + CH - 1) / CH;
  const bool mfma_ok = (Kdim % (bf16 ? 8 : 16) == 0) && ((uintptr_t)in % 16 == 0) && (NT == 1 || NT == 2 || NT == 4 || NT == 8);
  if (bf16)
    BFHIP_REQUIRE(mfma_ok, "spconv_gemm_bf16: needs K %% 8 == 0, N in {16,32,64,128} (padded), 16-byte aligned features");
  if (mfma_ok) {  // every check before the profiler scope opens and before the first launch
    if (workspace_bytes < bfhip_spconv_workspace_bytes(KV, Cin, Cout) || !workspace) {
      set_error("%s: workspace too small", name);
      return BFHIP_E_WORKSPACE;
    }
    BFHIP_REQUIRE(KV <= 32, "%s: kernel volume > 32 is not supported by the MFMA path", name);
  }
  ProfScope ps;
  prof_begin(transpose ? BFHIP_OP_SPCONV_BWD : BFHIP_OP_SPCONV_FWD, stream, &ps);
  // (A dense-style implicit GEMM for the wide layers -- 128-row tiles, the tile's pair table and both operands staged in LDS
  // by LDS-DMA, 32x32x16 MFMA, the dense conv's ring -- was built and measured: 64 -> 64: 43.9 vs 41.9 us, 128 -> 128: 75 vs
  // 71.6 us, strided data gradients up to 3x slower (their tables are ~1/8 full and every hole is a zero-page DMA + zero MFMA).
  // With ~190 row tiles the 128-channel stage leaves a quarter of the CUs idle either way; removed.)
  if (mfma_ok) {
    const dim3 pack_grid(ceil_div((long long)KV * CC * NT * 64 * KPL, 256));
    if (bf16)
      hipLaunchKernelGGL((pack_weights_kernel<__bf16, OpBf16<false>::KPL>), pack_grid, dim3(256), 0, stream, W, Cout, KV, Cin,
                         transpose, flip, CC, NT, (__bf16 *)workspace);
    else
      hipLaunchKernelGGL((pack_weights_kernel<float, OpF32::KPL>), pack_grid, dim3(256), 0, stream, W, Cout, KV, Cin, transpose,
                         flip, CC, NT, (float *)workspace);
    // rows per wave: aim for >= ~1024 workgroups (4 per CU); a workgroup covers 4*R*16 rows
    int R = n_rows >= 262144 ? 4 : (n_rows >= (bf16 ? 65536 : 131072) ? 2 : 1);
    if (!bf16 && NT == 8 && R == 4) R = 2;
    dispatch_tile(NT, R, io16, [&](auto nt, auto r, auto io) {
      auto launch = [&](auto kernel, auto *Wp) {
        hipLaunchKernelGGL(kernel, dim3(ceil_div(n_rows, 4 * r.value * 16)), dim3(256), 0, stream, in, Kdim, Wp, pairs, ld, KV,
                           n_rows, Ndim, perm, row_mask, out);
      };
      // measured on the encoder's layers (tools/gemm_micro.py, bf16 storage): 128 -> 128: 88.8 -> 79.4 us, 64 -> 128: 53.1 -> 46.5,
      // 64 -> 64: 53.2 -> 52.6; 32 -> 32: 48.1 -> 59.1 and 16 -> 32: 40.0 -> 59.8 (27 one-chunk steps: the up-front index fetch costs
      // more than the deeper pipeline saves), hence the split at 64 input channels
      if (!bf16)
        launch(spconv_gemm_kernel<OpF32, nt.value, r.value>, (const f32x4 *)workspace);
      else if (Kdim >= 64)
        launch(spconv_gemm_bf16p_kernel<nt.value, r.value, io.value>, (const bf16x8 *)workspace);
      else
        launch(spconv_gemm_kernel<OpBf16<io.value>, nt.value, r.value>, (const bf16x8 *)workspace);
    });
  } else {
    long long total = (long long)n_rows * Ndim;
    hipLaunchKernelGGL(spconv_scalar_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, stream, (const float *)in, Kdim, W, Cout,
                       Cin, transpose, flip, pairs, ld, KV, n_rows, Ndim, (float *)out);
  }
  prof_end(&ps);
  return check_launch(name);
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

// Gather-GEMM: out[n_rows, Ndim] = sum_k M_k . in[pairs[k][row]]  with M_k derived from W (Cout,KV,Cin):
//   transpose=0: forward  (Kdim = Cin,  Ndim = Cout)
//   transpose=1: dgrad    (Kdim = Cout, Ndim = Cin); flip=1 uses W[KV-1-k] (SubM with pair_fwd as pair_bwd)
BFHIP_EXPORT size_t bfhip_spconv_workspace_bytes(int KV, int Cin, int Cout) {
  size_t cc = (size_t)((Cin > Cout ? Cin : Cout) + 15) / 16;
  return align_up((size_t)KV * cc * cc * 64 * 4 * sizeof(float), 256) + 256;
}

BFHIP_EXPORT int bfhip_spconv_gemm(const float *in, const float *W, const int32_t *pairs, int ld, int KV,
                                   int n_rows, int Cin, int Cout, int transpose, int flip,
                                   const int32_t *perm, const uint32_t *row_mask, float *out,
                                   void *workspace, size_t workspace_bytes, void *stream_) {
  return spconv_gemm_impl(false, "spconv_gemm", in, W, pairs, ld, KV, n_rows, Cin, Cout, transpose, flip, perm, row_mask, out,
                          false, workspace, workspace_bytes, (hipStream_t)stream_);
}

// Same contract as bfhip_spconv_gemm with bf16 MFMA inputs (features/weights rounded to bf16 on load,
// fp32 accumulate and output): the bf16 configs (the reference runs spconv in half precision under AMP).
// Requires Kdim % 8 == 0; other shapes are rejected (use the fp32 entry point).
BFHIP_EXPORT int bfhip_spconv_gemm_bf16(const void *in, const float *W, const int32_t *pairs, int ld, int KV,
                                        int n_rows, int Cin, int Cout, int transpose, int flip,
                                        const int32_t *perm, const uint32_t *row_mask, void *out, int io_bf16,
                                        void *workspace, size_t workspace_bytes, void *stream_) {
  return spconv_gemm_impl(true, "spconv_gemm_bf16", in, W, pairs, ld, KV, n_rows, Cin, Cout, transpose, flip, perm, row_mask,
                          out, io_bf16 != 0, workspace, workspace_bytes, (hipStream_t)stream_);
}
