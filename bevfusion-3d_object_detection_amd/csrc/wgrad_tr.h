// wgrad_tr.h -- the machinery the dense (conv2d_wgrad.hip) and the sparse (spconv_wgrad_tr.hip) weight gradient share.
// dW[co][k] = sum over pixels of dy[m][co] * A[m][k].  LDS tiles are pixel-major: dy [64][128 co], A [64][128 k]
// (256-byte rows; piece c of row r at position c ^ (((r & 3) << 2) | ((r >> 2) & 3)), conflict-free for the
// transposing read).  ds_read_b64_tr_b16 hands each lane 4 consecutive pixels of ONE column: the K-major fragment the
// 32x32x16 MFMA wants, for both operands.  The pixel range is split over workgroups, each split writes an fp32 slab of dW,
// and the slabs are summed in a fixed order (wgrad_reduce_body).
#pragma once
#include "conv_common.h"

namespace bfhip {
namespace {

__device__ __forceinline__ int tr_swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// ---- shared by the dense and the sparse weight-gradient kernels: wave tile = 64 rows (wm) x 64 columns (wn) of dW;
// a 16-lane group reads a 4-pixel x 16-column block with the transposing LDS read
struct TrAddr { int g[2][2], x[2][2]; };  // [tile 0/1][half], for k-step 0; k-step ks adds ks * 16 rows (swizzle period 16)

__device__ __forceinline__ TrAddr tr_addresses(int lane, int wm, int wn) {
  const int grp = (lane >> 4) & 1, li = lane & 15, tq = li >> 2, tp = li & 3, lh = lane >> 5;
  TrAddr a;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int r = 8 * lh + 4 * half + tq;  // row inside a 16-pixel k-step
      const int cg = ((wm * 64 + j * 32) >> 3) + 2 * grp + (tp >> 1);
      const int cx = ((wn * 64 + j * 32) >> 3) + 2 * grp + (tp >> 1);
      a.g[j][half] = r * 256 + ((cg ^ tr_swz(r)) << 4) + 8 * (tp & 1);
      a.x[j][half] = r * 256 + ((cx ^ tr_swz(r)) << 4) + 8 * (tp & 1);
    }
  return a;
}

// LDS byte address of a pointer into the dynamic-LDS region
__device__ __forceinline__ unsigned lds_addr(const void *p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char *)p;
}

// Transposing LDS read as inline asm, NOT the builtin: behind a `global_load_lds` the compiler's wait-count pass puts an
// `s_waitcnt vmcnt(0)` in front of every `llvm.amdgcn.ds.read.tr16.b64` (it cannot tell the read from the DMA's destination),
// which drains the prefetched stages before the first read of each step -- DMA and MFMAs then never overlap inside a
// workgroup (round 2's kernels ran that way: 30 % MFMA-busy at any tile size or ring depth).  With asm reads the order is
// ours to keep: counted vmcnt + raw s_barrier before the reads, lgkmcnt(0) (tied to the destination registers, so that the
// MFMAs cannot be scheduled above it) before their use.
template <int OFF>
__device__ __forceinline__ short4_t lds_read_tr(unsigned addr) {
  short4_t v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

__device__ __forceinline__ void lds_wait_all(short4_t (&a)[2][2][2], short4_t (&b)[2][2][2]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0][0][0]), "+v"(a[0][0][1]), "+v"(a[0][1][0]), "+v"(a[0][1][1]), "+v"(a[1][0][0]), "+v"(a[1][0][1]),
                 "+v"(a[1][1][0]), "+v"(a[1][1][1]), "+v"(b[0][0][0]), "+v"(b[0][0][1]), "+v"(b[0][1][0]), "+v"(b[0][1][1]),
                 "+v"(b[1][0][0]), "+v"(b[1][0][1]), "+v"(b[1][1][0]), "+v"(b[1][1][1])
               :
               : "memory");
}

// one 64-pixel step: acc[i][j] += G^T(tile i) . X(tile j).  Reads of k-steps 2-3 are in flight under the MFMAs of k-steps 0-1.
__device__ __forceinline__ void tr_compute_step(const unsigned char *pG, const unsigned char *pX, const TrAddr &ad, f32x16 (&acc)[2][2]) {
  typedef __attribute__((ext_vector_type(8))) short short8_t;
  const unsigned aG = lds_addr(pG), aX = lds_addr(pX);
  short4_t g0[2][2][2], x0[2][2][2], g1[2][2][2], x1[2][2][2];  // [k-step of the pair][tile j][half]
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      g0[0][j][h] = lds_read_tr<0>(aG + ad.g[j][h]);
      x0[0][j][h] = lds_read_tr<0>(aX + ad.x[j][h]);
      g0[1][j][h] = lds_read_tr<16 * 256>(aG + ad.g[j][h]);
      x0[1][j][h] = lds_read_tr<16 * 256>(aX + ad.x[j][h]);
    }
  lds_wait_all(g0, x0);
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      g1[0][j][h] = lds_read_tr<32 * 256>(aG + ad.g[j][h]);
      x1[0][j][h] = lds_read_tr<32 * 256>(aX + ad.x[j][h]);
      g1[1][j][h] = lds_read_tr<48 * 256>(aG + ad.g[j][h]);
      x1[1][j][h] = lds_read_tr<48 * 256>(aX + ad.x[j][h]);
    }
  auto mfma_pair = [&](short4_t (&g)[2][2][2], short4_t (&x)[2][2][2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        short8_t av = {g[ks][j][0][0], g[ks][j][0][1], g[ks][j][0][2], g[ks][j][0][3], g[ks][j][1][0], g[ks][j][1][1], g[ks][j][1][2], g[ks][j][1][3]};
        short8_t bv = {x[ks][j][0][0], x[ks][j][0][1], x[ks][j][0][2], x[ks][j][0][3], x[ks][j][1][0], x[ks][j][1][1], x[ks][j][1][2], x[ks][j][1][3]};
        a[j] = __builtin_bit_cast(bf16x8, av);
        b[j] = __builtin_bit_cast(bf16x8, bv);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };
  mfma_pair(g0, x0);
  lds_wait_all(g1, x1);
  mfma_pair(g1, x1);
}

// partial slab [Cout][Ktot] (fp32) of one split: rows = co, lanes = k columns (contiguous)
__device__ __forceinline__ void tr_store_slab(float *out, int Cout, int Ktot, int co0, int q0, int lane, int wm, int wn,
                                              const f32x16 (&acc)[2][2]) {
  const int lh = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = q0 * 8 + wn * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (co < Cout && col < Ktot) out[(size_t)co * Ktot + col] = acc[i][j][r];
      }
    }
}

// dW = sum over splits (fixed order), written as fp32 or bf16.  The loads of 8 slabs are issued before their adds: one
// dependent round trip per 8 slabs instead of one per slab (18 slabs of the 128 -> 128 sparse layers: 31 -> ~8 us).
__device__ __forceinline__ void wgrad_reduce_body(const float *__restrict__ slab, int splits, long long total,
                                                  void *__restrict__ dw, int out_bf16, long long block) {
  long long i = (block * 256 + threadIdx.x) * 4;
  if (i >= total) return;
  if (i + 4 <= total) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = 0;
    for (; k + 8 <= splits; k += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *(const float4 *)(slab + (size_t)(k + u) * total + i);
#pragma unroll
      for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    for (; k < splits; ++k) {
      float4 v = *(const float4 *)(slab + (size_t)k * total + i);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (out_bf16) {
      uint2 o;
      o.x = bf16_rne(s.x) | (bf16_rne(s.y) << 16);
      o.y = bf16_rne(s.z) | (bf16_rne(s.w) << 16);
      *(uint2 *)((bf16_t *)dw + i) = o;
    } else *(float4 *)((float *)dw + i) = s;
  } else {
    for (long long e = i; e < total; ++e) {
      float a = 0.f;
      for (int k = 0; k < splits; ++k) a += slab[(size_t)k * total + e];
      if (out_bf16) ((bf16_t *)dw)[e] = (bf16_t)bf16_rne(a);
      else ((float *)dw)[e] = a;
    }
  }
}

}  // namespace
}  // namespace bfhip
