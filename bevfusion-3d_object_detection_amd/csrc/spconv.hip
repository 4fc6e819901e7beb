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
// Compute :  output-stationary implicit GEMM on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32):
//            one wave owns R*16 output rows x all C_out columns, loops over the KV offsets,
//            skips offsets none of its rows has, gathers A rows straight from L2 with one 16-B
//            load per lane (K permuted consistently in the pre-packed weights, so no shuffle),
//            no atomics -> deterministic.  The same kernel computes dgrad (weights transposed,
//            pair_bwd).  wgrad: wave per (offset, row split, tile group), K = rows, partial slabs
//            reduced in a fixed order.
#include "spconv_common.h"

namespace bfhip {
namespace {

// -------------------------------------------------------------------------------- weight packing
// Wp[((k*CC + cc)*NT + nt)*64 + lane][j] = M_k[cc*16 + 4*(lane>>4) + j][nt*16 + (lane&15)]
//   forward : M_k[ci][co] = W[co][k][ci]                      (K = C_in,  N = C_out)
//   dgrad   : M_k[co][ci] = W[co][flip ? KV-1-k : k][ci]      (K = C_out, N = C_in)
__global__ __launch_bounds__(256) void pack_weights_kernel(const float *__restrict__ W, int Cout,
                                                           int KV, int Cin, int transpose, int flip,
                                                           int CC, int NT, float *__restrict__ Wp) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)KV * CC * NT * 64 * 4;
  if (t >= total) return;
  int j = (int)(t & 3);
  int lane = (int)((t >> 2) & 63);
  long long r = t >> 8;
  int nt = (int)(r % NT); r /= NT;
  int cc = (int)(r % CC);
  int k = (int)(r / CC);
  int kk = cc * 16 + 4 * (lane >> 4) + j;  // K index
  int nn = nt * 16 + (lane & 15);          // N index
  float v = 0.f;
  if (!transpose) {
    if (kk < Cin && nn < Cout) v = W[((size_t)nn * KV + k) * Cin + kk];
  } else {
    int ks = flip ? KV - 1 - k : k;
    if (kk < Cout && nn < Cin) v = W[((size_t)kk * KV + ks) * Cin + nn];
  }
  Wp[t] = v;
}

// -------------------------------------------------------------------------------- forward / dgrad
// Workgroup version: 4 waves share every weight tile through LDS (double buffered, one barrier per
// (offset, 16-channel chunk) step); the workgroup skips offsets none of its 4*R*16 rows uses.
// Weight traffic from L2 drops 4x versus one weight fetch per wave; A rows are still gathered per wave.
template <int NT, int R>
__global__ __launch_bounds__(256) void spconv_gemm_lds_kernel(const float *__restrict__ in, int Kdim,
                                                              const f32x4 *__restrict__ Wp,
                                                              const int *__restrict__ pairs, int ld,
                                                              int KV, int n_rows, int Ndim,
                                                              const int *__restrict__ perm,
                                                              const unsigned *__restrict__ row_mask,
                                                              float *__restrict__ out) {
  __shared__ f32x4 sB[2][NT * 64];
  __shared__ unsigned s_mask;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  // XCD-chunked block order (common.h): each XCD walks one contiguous eighth of the (region-major sorted) rows
  const long long row_base = (xcd_chunked_block(blockIdx.x, gridDim.x) * 4 + wv) * (R * 16);
  const int lr = lane & 15, lq = lane >> 4;
  const int CC = Kdim >> 4;
  if (tid == 0) s_mask = 0u;
  __syncthreads();
  // rows of this wave: position in mask-sorted order -> actual row
  int my_row[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    long long sp = row_base + r * 16 + lr;
    my_row[r] = sp < n_rows ? (perm ? perm[sp] : (int)sp) : -1;
  }
  // which offsets does this wave / workgroup need
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
      for (int r = 0; r < R; ++r) any |= (my_row[r] >= 0) && (pairs[(size_t)k * ld + my_row[r]] >= 0);
      if (__any(any)) wmask |= 1u << k;
    }
  }
  if (lane == 0 && wmask) atomicOr(&s_mask, wmask);
  __syncthreads();
  unsigned gmask = s_mask;

  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int LOADS = (NT * 64 + 255) / 256;  // float4 per thread per weight tile
  f32x4 pre[LOADS];
  auto prefetch = [&](int k, int cc) {
    const f32x4 *wp = Wp + ((size_t)(k * CC + cc) * NT) * 64;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      int e = tid + i * 256;
      if (e < NT * 64) pre[i] = wp[e];
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      int e = tid + i * 256;
      if (e < NT * 64) sB[buf][e] = pre[i];
    }
  };
  auto next_set = [&](int kk) {  // next offset the workgroup needs after kk (KV if none)
    unsigned rest = gmask & ~((2u << kk) - 1u);
    return rest ? __ffs(rest) - 1 : KV;
  };
  auto load_idx = [&](int kk, int *dst) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      dst[r] = (kk < KV && my_row[r] >= 0 && ((wmask >> kk) & 1u)) ? pairs[(size_t)kk * ld + my_row[r]] : -1;
  };
  auto gather = [&](const int *ix, int c, f32x4 *dst) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      dst[r] = ix[r] >= 0 ? *(const f32x4 *)(in + (size_t)ix[r] * Kdim + c * 16 + lq * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
  };
  // software pipeline: weight tile i+1 (global->regs->LDS), A rows of step i+1 and the pair indices of
  // the NEXT offset are all in flight while the MFMAs of step i run
  int k = gmask ? __ffs(gmask) - 1 : KV;
  int cc = 0, buf = 0;
  int idx[R], idx_nxt[R];
  f32x4 a[R], a_nxt[R];
  if (k < KV) {
    prefetch(k, 0);
    load_idx(k, idx);
    load_idx(next_set(k), idx_nxt);
    gather(idx, 0, a);
  }
  while (k < KV) {
    stash(buf);
    __syncthreads();
    int nk = k, ncc = cc + 1;
    if (ncc == CC) { ncc = 0; nk = next_set(k); }
    if (nk < KV) {
      prefetch(nk, ncc);
      gather(ncc == 0 ? idx_nxt : idx, ncc, a_nxt);
    }
    if ((wmask >> k) & 1u) {
      f32x4 b[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) b[nt] = sB[buf][nt * 64 + lane];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r][j], b[nt][j], acc[r][nt], 0, 0, 0);
    }
    if (ncc == 0 && nk < KV) {  // moving on to offset nk: rotate the index registers, fetch the one after
#pragma unroll
      for (int r = 0; r < R; ++r) idx[r] = idx_nxt[r];
      load_idx(next_set(nk), idx_nxt);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = a_nxt[r];
    k = nk;
    cc = ncc;
    buf ^= 1;
  }
  // C/D layout: col = lane&15, row = (lane>>4)*4 + i ; the actual output row lives in lane (lq*4+i) of my_row
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int row = __shfl(my_row[r], lq * 4 + i);
      if (row >= 0) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          int col = nt * 16 + lr;
          if (col < Ndim) out[(size_t)row * Ndim + col] = acc[r][nt][i];
        }
      }
    }
}

// ---- bf16-input variant (fp32 features in HBM, converted on load; fp32 accumulate): for the bf16 configs.
// v_mfma_f32_16x16x32_bf16: lane l supplies A[row = l&15][k = 8*(l>>4) + j], B[k = 8*(l>>4) + j][col = l&15], j < 8,
// so one step covers 32 input channels (two float4 gathers per lane and row tile) with ONE MFMA per tile.
// Wp16[((k*CC32 + c32)*NT + nt)*64 + lane][j] = bf16(M_k[c32*32 + 8*(lane>>4) + j][nt*16 + (lane&15)])
__global__ __launch_bounds__(256) void pack_weights_bf16_kernel(const float *__restrict__ W, int Cout,
                                                                int KV, int Cin, int transpose, int flip,
                                                                int CC32, int NT, __bf16 *__restrict__ Wp) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)KV * CC32 * NT * 64 * 8;
  if (t >= total) return;
  int j = (int)(t & 7);
  int lane = (int)((t >> 3) & 63);
  long long r = t >> 9;
  int nt = (int)(r % NT); r /= NT;
  int c32 = (int)(r % CC32);
  int k = (int)(r / CC32);
  int kk = c32 * 32 + 8 * (lane >> 4) + j;
  int nn = nt * 16 + (lane & 15);
  float v = 0.f;
  if (!transpose) {
    if (kk < Cin && nn < Cout) v = W[((size_t)nn * KV + k) * Cin + kk];
  } else {
    int ks = flip ? KV - 1 - k : k;
    if (kk < Cout && nn < Cin) v = W[((size_t)kk * KV + ks) * Cin + nn];
  }
  Wp[t] = (__bf16)v;
}

template <int NT, int R, bool IO16>
__global__ __launch_bounds__(256) void spconv_gemm_bf16_kernel(const void *__restrict__ in_, int Kdim,
                                                               const bf16x8 *__restrict__ Wp,
                                                               const int *__restrict__ pairs, int ld,
                                                               int KV, int n_rows, int Ndim,
                                                               const int *__restrict__ perm,
                                                               const unsigned *__restrict__ row_mask,
                                                               void *__restrict__ out_) {
  // IO16: features stored in bf16 (gathered rows are the MFMA operand as they are: one 16-byte load per lane and step,
  // half the gather traffic of fp32 storage) and the output rounded to bf16 once; otherwise fp32 in / fp32 out.
  const float *in = (const float *)in_;
  const __bf16 *in16 = (const __bf16 *)in_;
  float *out = (float *)out_;
  __bf16 *out16 = (__bf16 *)out_;
  __shared__ bf16x8 sB[2][NT * 64];
  __shared__ unsigned s_mask;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  // XCD-chunked block order (common.h): each XCD walks one contiguous eighth of the (region-major sorted) rows
  const long long row_base = (xcd_chunked_block(blockIdx.x, gridDim.x) * 4 + wv) * (R * 16);
  const int lr = lane & 15, lq = lane >> 4;
  const int CC = (Kdim + 31) >> 5;
  if (tid == 0) s_mask = 0u;
  __syncthreads();
  int my_row[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    long long sp = row_base + r * 16 + lr;
    my_row[r] = sp < n_rows ? (perm ? perm[sp] : (int)sp) : -1;
  }
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
      for (int r = 0; r < R; ++r) any |= (my_row[r] >= 0) && (pairs[(size_t)k * ld + my_row[r]] >= 0);
      if (__any(any)) wmask |= 1u << k;
    }
  }
  if (lane == 0 && wmask) atomicOr(&s_mask, wmask);
  __syncthreads();
  unsigned gmask = s_mask;

  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int LOADS = (NT * 64 + 255) / 256;
  bf16x8 pre[LOADS];
  auto prefetch = [&](int k, int cc) {
    const bf16x8 *wp = Wp + ((size_t)(k * CC + cc) * NT) * 64;
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      int e = tid + i * 256;
      if (e < NT * 64) pre[i] = wp[e];
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      int e = tid + i * 256;
      if (e < NT * 64) sB[buf][e] = pre[i];
    }
  };
  auto next_set = [&](int kk) {
    unsigned rest = gmask & ~((2u << kk) - 1u);
    return rest ? __ffs(rest) - 1 : KV;
  };
  auto load_idx = [&](int kk, int *dst) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      dst[r] = (kk < KV && my_row[r] >= 0 && ((wmask >> kk) & 1u)) ? pairs[(size_t)kk * ld + my_row[r]] : -1;
  };
  auto gather = [&](const int *ix, int c, f32x4 *lo, f32x4 *hi) {
    const int ch = c * 32 + lq * 8;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (ix[r] >= 0 && ch < Kdim) {
        if (IO16) {
          lo[r] = *(const f32x4 *)(in16 + (size_t)ix[r] * Kdim + ch);  // 8 bf16 carried in one 16-byte register group
          hi[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
        } else {
          const float *src = in + (size_t)ix[r] * Kdim + ch;
          lo[r] = *(const f32x4 *)src;
          hi[r] = *(const f32x4 *)(src + 4);
        }
      } else {
        lo[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
        hi[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  int k = gmask ? __ffs(gmask) - 1 : KV;
  int cc = 0, buf = 0;
  int idx[R], idx_nxt[R];
  f32x4 alo[R], ahi[R], nlo[R], nhi[R];
  if (k < KV) {
    prefetch(k, 0);
    load_idx(k, idx);
    load_idx(next_set(k), idx_nxt);
    gather(idx, 0, alo, ahi);
  }
  while (k < KV) {
    stash(buf);
    __syncthreads();
    int nk = k, ncc = cc + 1;
    if (ncc == CC) { ncc = 0; nk = next_set(k); }
    if (nk < KV) {
      prefetch(nk, ncc);
      gather(ncc == 0 ? idx_nxt : idx, ncc, nlo, nhi);
    }
    if ((wmask >> k) & 1u) {
      bf16x8 a[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (IO16) {
          a[r] = __builtin_bit_cast(bf16x8, alo[r]);
        } else {
          a[r][0] = (__bf16)alo[r][0]; a[r][1] = (__bf16)alo[r][1]; a[r][2] = (__bf16)alo[r][2]; a[r][3] = (__bf16)alo[r][3];
          a[r][4] = (__bf16)ahi[r][0]; a[r][5] = (__bf16)ahi[r][1]; a[r][6] = (__bf16)ahi[r][2]; a[r][7] = (__bf16)ahi[r][3];
        }
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        bf16x8 b = sB[buf][nt * 64 + lane];
#pragma unroll
        for (int r = 0; r < R; ++r)
          acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[r], b, acc[r][nt], 0, 0, 0);
      }
    }
    if (ncc == 0 && nk < KV) {
#pragma unroll
      for (int r = 0; r < R; ++r) idx[r] = idx_nxt[r];
      load_idx(next_set(nk), idx_nxt);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) { alo[r] = nlo[r]; ahi[r] = nhi[r]; }
    k = nk;
    cc = ncc;
    buf ^= 1;
  }
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
            if (IO16) out16[(size_t)row * Ndim + col] = (__bf16)acc[r][nt][i];
            else out[(size_t)row * Ndim + col] = acc[r][nt][i];
          }
        }
      }
    }
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

// Pipelined variant of spconv_gemm_bf16_kernel: the same tiling (workgroup = 4 waves x R x 16 output rows, all NT column
// tiles, one (offset, 32-channel chunk) per step with the weight tile shared through LDS), restructured around latency.
// The original issued the gathers and the weight-tile loads of step s+1 during step s: one step is only NT * R MFMAs
// (0.1-0.4 us), so most of every ~1 us round trip was exposed, 27 * CC times per workgroup.  Here
//  * all pair-table entries of the workgroup's rows are fetched once, back to back, into LDS (s_idx) -- no dependent
//    index load remains inside the loop;
//  * loads run TWO steps ahead: three register sets used cyclically (the loop is unrolled by 3 so that no set is copied
//    while its loads are in flight), gathers are unconditional from clamped addresses and masked when consumed.
template <int NT, int R, bool IO16>
__global__ __launch_bounds__(256) void spconv_gemm_bf16p_kernel(const void *__restrict__ in_, int Kdim,
                                                                const bf16x8 *__restrict__ Wp,
                                                                const int *__restrict__ pairs, int ld,
                                                                int KV, int n_rows, int Ndim,
                                                                const int *__restrict__ perm,
                                                                const unsigned *__restrict__ row_mask,
                                                                void *__restrict__ out_) {
  const float *in = (const float *)in_;
  const __bf16 *in16 = (const __bf16 *)in_;
  float *out = (float *)out_;
  __bf16 *out16 = (__bf16 *)out_;
  __shared__ bf16x8 sB[2][NT * 64];
  __shared__ unsigned s_mask;
  __shared__ int s_idx[4][32][16 * R];  // [wave][offset][row of the wave]; KV <= 32 (checked by the host)
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  // XCD-chunked block order (common.h): each XCD walks one contiguous eighth of the (region-major sorted) rows
  const long long row_base = (xcd_chunked_block(blockIdx.x, gridDim.x) * 4 + wv) * (R * 16);
  const int lr = lane & 15, lq = lane >> 4;
  const int CC = (Kdim + 31) >> 5;
  if (tid == 0) s_mask = 0u;
  __syncthreads();
  int my_row[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    long long sp = row_base + r * 16 + lr;
    my_row[r] = sp < n_rows ? (perm ? perm[sp] : (int)sp) : -1;
  }
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
      for (int r = 0; r < R; ++r) any |= s_idx[wv][k][r * 16 + lr] >= 0;
      if (__any(any)) wmask |= 1u << k;
    }
  }
  if (lane == 0 && wmask) atomicOr(&s_mask, wmask);
  __syncthreads();
  const unsigned gmask = s_mask;

  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int LOADS = (NT * 64 + 255) / 256;
  struct Set {  // what one step needs from memory
    bf16x8 pre[LOADS];
    f32x4 lo[R], hi[R];
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
      st.pre[i] = wp[e < NT * 64 ? e : 0];
    }
    const int ch = cc * 32 + lq * 8;
    const int chc = ch < Kdim ? ch : 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int ix = s_idx[wv][k][r * 16 + lr];
      st.ix[r] = ch < Kdim ? ix : -1;
      const size_t off = (size_t)max(ix, 0) * Kdim + chc;
      if (IO16) {
        st.lo[r] = *(const f32x4 *)(in16 + off);  // 8 bf16 carried in one 16-byte register group
      } else {
        st.lo[r] = *(const f32x4 *)(in + off);
        st.hi[r] = *(const f32x4 *)(in + off + 4);
      }
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
      for (int r = 0; r < R; ++r) {
        if (IO16) {
          a[r] = __builtin_bit_cast(bf16x8, cur.ix[r] >= 0 ? cur.lo[r] : (f32x4){0.f, 0.f, 0.f, 0.f});
        } else {
          const f32x4 l = cur.ix[r] >= 0 ? cur.lo[r] : (f32x4){0.f, 0.f, 0.f, 0.f};
          const f32x4 h = cur.ix[r] >= 0 ? cur.hi[r] : (f32x4){0.f, 0.f, 0.f, 0.f};
          a[r][0] = (__bf16)l[0]; a[r][1] = (__bf16)l[1]; a[r][2] = (__bf16)l[2]; a[r][3] = (__bf16)l[3];
          a[r][4] = (__bf16)h[0]; a[r][5] = (__bf16)h[1]; a[r][6] = (__bf16)h[2]; a[r][7] = (__bf16)h[3];
        }
      }
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
            if (IO16) out16[(size_t)row * Ndim + col] = (__bf16)acc[r][nt][i];
            else out[(size_t)row * Ndim + col] = acc[r][nt][i];
          }
        }
      }
    }
}

// Launchers: NT in {1, 2, 4, 8} column tiles, R in {1, 2, 4} row tiles per wave (validated / chosen by the entry points);
// one workgroup = 4 waves x R*16 rows.
void launch_gemm(int NT, int R, hipStream_t stream, const float *in, int Kdim, const f32x4 *Wp, const int *pairs, int ld,
                 int KV, int n_rows, int Ndim, const int *perm, const unsigned *row_mask, float *out) {
  dispatch_tile(NT, R, false, [&](auto nt, auto r, auto) {
    hipLaunchKernelGGL((spconv_gemm_lds_kernel<nt.value, r.value>), dim3(ceil_div(n_rows, 4 * r.value * 16)), dim3(256), 0,
                       stream, in, Kdim, Wp, pairs, ld, KV, n_rows, Ndim, perm, row_mask, out);
  });
}

void launch_gemm_bf16(int NT, int R, bool io16, hipStream_t stream, const void *in, int Kdim, const bf16x8 *Wp,
                      const int *pairs, int ld, int KV, int n_rows, int Ndim, const int *perm, const unsigned *row_mask,
                      void *out) {
  dispatch_tile(NT, R, io16, [&](auto nt, auto r, auto io) {
    const dim3 grid(ceil_div(n_rows, 4 * r.value * 16));
    // measured on the encoder's layers (tools/gemm_micro.py, bf16 storage): 128 -> 128: 88.8 -> 79.4 us, 64 -> 128: 53.1 -> 46.5,
    // 64 -> 64: 53.2 -> 52.6; 32 -> 32: 48.1 -> 59.1 and 16 -> 32: 40.0 -> 59.8 (27 one-chunk steps: the up-front index fetch costs
    // more than the deeper pipeline saves), hence the split at 64 input channels
    if (Kdim >= 64)
      hipLaunchKernelGGL((spconv_gemm_bf16p_kernel<nt.value, r.value, io.value>), grid, dim3(256), 0, stream, in, Kdim, Wp, pairs,
                         ld, KV, n_rows, Ndim, perm, row_mask, out);
    else
      hipLaunchKernelGGL((spconv_gemm_bf16_kernel<nt.value, r.value, io.value>), grid, dim3(256), 0, stream, in, Kdim, Wp, pairs,
                         ld, KV, n_rows, Ndim, perm, row_mask, out);
  });
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
  hipStream_t stream = (hipStream_t)stream_;
  BFHIP_REQUIRE(KV > 0 && Cin > 0 && Cout > 0 && n_rows >= 0 && ld >= n_rows, "spconv_gemm: bad sizes");
  if (n_rows == 0) return BFHIP_OK;
  BFHIP_REQUIRE(in && W && pairs && out, "spconv_gemm: null pointer");
  int Kdim = transpose ? Cout : Cin, Ndim = transpose ? Cin : Cout;
  int NT = (Ndim + 15) / 16, CC = (Kdim + 15) / 16;
  bool mfma_ok = (Kdim % 16 == 0) && ((uintptr_t)in % 16 == 0) && (NT == 1 || NT == 2 || NT == 4 || NT == 8);
  if (mfma_ok) {  // every check before the profiler scope opens and before the first launch
    BFHIP_REQUIRE_WORKSPACE(workspace, workspace_bytes, bfhip_spconv_workspace_bytes(KV, Cin, Cout), "spconv_gemm");
    BFHIP_REQUIRE(KV <= 32, "spconv_gemm: kernel volume > 32 is not supported by the MFMA path");
  }
  ProfScope ps;
  prof_begin(transpose ? BFHIP_OP_SPCONV_BWD : BFHIP_OP_SPCONV_FWD, stream, &ps);
  if (mfma_ok) {
    float *Wp = (float *)workspace;
    long long total = (long long)KV * CC * NT * 256;
    hipLaunchKernelGGL(pack_weights_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, stream, W, Cout, KV, Cin, transpose,
                       flip, CC, NT, Wp);
    // rows per wave: aim for >= ~1024 workgroups (4 per CU); a workgroup covers 4*R*16 rows
    int R = n_rows >= 262144 ? 4 : (n_rows >= 131072 ? 2 : 1);
    if (NT == 8 && R == 4) R = 2;
    launch_gemm(NT, R, stream, in, Kdim, (const f32x4 *)Wp, pairs, ld, KV, n_rows, Ndim, perm, row_mask, out);
  } else {
    long long total = (long long)n_rows * Ndim;
    hipLaunchKernelGGL(spconv_scalar_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, stream, in, Kdim, W, Cout, Cin,
                       transpose, flip, pairs, ld, KV, n_rows, Ndim, out);
  }
  prof_end(&ps);
  return check_launch("spconv_gemm");
}

// Same contract as bfhip_spconv_gemm with bf16 MFMA inputs (features/weights rounded to bf16 on load,
// fp32 accumulate and output): the bf16 configs (the reference runs spconv in half precision under AMP).
// Requires Kdim % 8 == 0; other shapes are rejected (use the fp32 entry point).
BFHIP_EXPORT int bfhip_spconv_gemm_bf16(const void *in, const float *W, const int32_t *pairs, int ld, int KV,
                                        int n_rows, int Cin, int Cout, int transpose, int flip,
                                        const int32_t *perm, const uint32_t *row_mask, void *out, int io_bf16,
                                        void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BFHIP_REQUIRE(KV > 0 && KV <= 32 && Cin > 0 && Cout > 0 && n_rows >= 0 && ld >= n_rows, "spconv_gemm_bf16: bad sizes");
  if (n_rows == 0) return BFHIP_OK;
  BFHIP_REQUIRE(in && W && pairs && out, "spconv_gemm_bf16: null pointer");
  int Kdim = transpose ? Cout : Cin, Ndim = transpose ? Cin : Cout;
  int NT = (Ndim + 15) / 16, CC32 = (Kdim + 31) / 32;
  BFHIP_REQUIRE(Kdim % 8 == 0 && ((uintptr_t)in % 16 == 0) && (NT == 1 || NT == 2 || NT == 4 || NT == 8),
                "spconv_gemm_bf16: needs K %% 8 == 0, N in {16,32,64,128} (padded), 16-byte aligned features");
  BFHIP_REQUIRE_WORKSPACE(workspace, workspace_bytes, bfhip_spconv_workspace_bytes(KV, Cin, Cout), "spconv_gemm_bf16");
  __bf16 *Wp = (__bf16 *)workspace;
  ProfScope ps;
  prof_begin(transpose ? BFHIP_OP_SPCONV_BWD : BFHIP_OP_SPCONV_FWD, stream, &ps);
  // (A dense-style implicit GEMM for the wide layers -- 128-row tiles, the tile's pair table and both operands staged in LDS
  // by LDS-DMA, 32x32x16 MFMA, the dense conv's ring -- was built and measured: 64 -> 64: 43.9 vs 41.9 us, 128 -> 128: 75 vs
  // 71.6 us, strided data gradients up to 3x slower (their tables are ~1/8 full and every hole is a zero-page DMA + zero MFMA).
  // With ~190 row tiles the 128-channel stage leaves a quarter of the CUs idle either way; removed.)
  long long total = (long long)KV * CC32 * NT * 512;
  hipLaunchKernelGGL(pack_weights_bf16_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, stream, W, Cout, KV, Cin, transpose,
                     flip, CC32, NT, Wp);
  int R = n_rows >= 262144 ? 4 : (n_rows >= 65536 ? 2 : 1);
  launch_gemm_bf16(NT, R, io_bf16 != 0, stream, in, Kdim, (const bf16x8 *)Wp, pairs, ld, KV, n_rows, Ndim, perm, row_mask, out);
  prof_end(&ps);
  return check_launch("spconv_gemm_bf16");
}
