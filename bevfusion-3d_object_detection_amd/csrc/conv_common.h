// conv_common.h -- what conv2d.hip, conv2d_wgrad.hip and spconv_wgrad_tr.hip share: operand types, the zero page, the gather
// geometry with its host-side builders, the tap table, output size and split planner.  Everything sits in an anonymous
// namespace: each unit has its own copy, the 64 KB zero page included.
#pragma once
#include "common.h"
#include <stddef.h>

namespace bfhip {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short short4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// Source of every padded / out-of-range / hole piece.  64 KB, and a wave reads from ITS OWN 64-byte line of it (zero_src()):
// with a single shared line every hole of every workgroup was a request to the same L2 channel -- at ~1 request per clock
// that one channel set the pace of the sparse kernels, where half of the pieces are holes (128 -> 128 SubM layer: 72 us with
// one line, whatever the prefetch depth).
constexpr int kZeroLines = 1024;
__device__ __attribute__((aligned(4096))) unsigned g_zero_page[kZeroLines * 16];

__device__ __forceinline__ const unsigned short *zero_src() {
  const unsigned line = (blockIdx.x * 8u + (threadIdx.x >> 6)) & (unsigned)(kZeroLines - 1);
  return (const unsigned short *)(g_zero_page + line * 16u);
}

struct ConvGeom {
  // gathered tensor [N, H, W, C] (pixel pitch ldx elements); GEMM rows = pixels of an [N, OH, OW] grid
  int N, H, W, C, ldx;
  int OH, OW;
  int KH, KW, stride, pad, dil;
  int transposed;  // 0: src = row * stride - pad + k * dil     1: t = row + pad - k * dil, src = t / stride if divisible
  int sshift, smask;  // transposed mode: stride = 1 << sshift, smask = stride - 1
  int nq;          // KH * KW * C / 8: number of 16-byte pieces along K
  long long M;     // N * OH * OW
  int Kout;        // GEMM columns (output channels of this GEMM)
  int ldw;         // weight row pitch in elements (= KH * KW * C)
  int ldy;         // output pixel pitch in elements
  // parity-class data gradient (MODE 2): class c owns row tiles [cls[c].tile0, cls[c + 1].tile0); its rows are the pixels
  // (h0 + i * stride, w0 + j * stride), i < Hc, j < Wc, of every image, and only the taps kh = kh0 + a * stride (a < nkh),
  // kw = kw0 + b * stride (b < nkw) reach them (none: nkh * nkw = 0, the class's gradient is zero)
  struct ParityClass { int h0, w0, Hc, Wc, kh0, kw0, nkh, nkw, tile0; } cls[17];
  int ncls;
};

__device__ __forceinline__ void glds16(const void *src, void *lds_dst) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1))) *)src,
                                   (void __attribute__((address_space(3))) *)lds_dst, 16, 0, 0);
}

// tap table: piece q -> (kh * dil) << 24 | (kw * dil) << 16 | ci
__device__ __forceinline__ void build_tap_table(unsigned *taps, const ConvGeom &g) {
  for (int q = threadIdx.x; q < g.nq; q += blockDim.x) {
    int k = q * 8;
    int tap = k / g.C, ci = k - tap * g.C;
    int kh = tap / g.KW, kw = tap - kh * g.KW;
    taps[q] = ((unsigned)(kh * g.dil) << 24) | ((unsigned)(kw * g.dil) << 16) | (unsigned)ci;
  }
}

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// K pieces (16-byte = 8-channel pieces of one tap) a kernel can hold a tap table for: 4 bytes per piece beside 64 KB of
// stages under the 80 KB dynamic-LDS attribute of the two-workgroups-per-CU tiles (the 256-wide tiles have 31 KB beside
// 128 KB, the wide weight-gradient tiles 16 KB beside 144 KB).  C is Cin for forward / weight gradient and Cout for the data
// gradient, so bfhip_conv2d_supported checks both (round 2 checked Cin only and allowed 8192 pieces: such calls passed
// `supported` and then failed at launch instead of falling back to the library).
constexpr int kMaxPieces = 3584;
inline bool geom_ok(int N, int H, int W, int C, int KH, int KW, int stride, int pad, int dil) {
  return N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && C < 65536 && KH > 0 && KW > 0 && stride > 0 &&
         (stride & (stride - 1)) == 0 /* the data gradient shifts instead of dividing */ && pad >= 0 && dil > 0 &&
         (KH - 1) * dil < 256 && (KW - 1) * dil < 256 && (long long)KH * KW * C / 8 <= kMaxPieces;
}

// ------------------------------------------------------------------------------------------------ host side
inline int conv_out_dim(int in, int k, int stride, int pad, int dil) { return (in + 2 * pad - dil * (k - 1) - 1) / stride + 1; }

// what the DMA asks of an operand it gathers: 16-byte aligned base, pixel pitch a multiple of 8 elements and >= its channels
inline bool dma_operand_ok(const void *p, int ld, int C) { return ((uintptr_t)p % 16) == 0 && ld % 8 == 0 && ld >= C; }
constexpr const char *kOperandMsg = "%s: operands must be 16-byte aligned with pitches that are multiples of 8 elements";

// forward-mode geometry (forward and weight gradient): gathered tensor = x [N, H, W, Cin], rows = output pixels
inline ConvGeom conv_geom_fwd(int N, int H, int W, int Cin, int ldx, int Cout, int KH, int KW, int stride, int pad, int dil,
                              int ldy) {
  ConvGeom g = {};
  g.N = N; g.H = H; g.W = W; g.C = Cin; g.ldx = ldx;
  g.OH = conv_out_dim(H, KH, stride, pad, dil);
  g.OW = conv_out_dim(W, KW, stride, pad, dil);
  g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad; g.dil = dil;
  g.nq = KH * KW * Cin / 8;
  g.M = (long long)N * g.OH * g.OW;
  g.Kout = Cout; g.ldw = KH * KW * Cin; g.ldy = ldy;
  return g;
}

// transposed-mode geometry (data gradient of the convolution x [N, H, W, Cin] -> dy [N, OH, OW, Cout]): gathered tensor = dy,
// rows = input pixels, stride a power of two.  `parity`: split the rows of a strided layer into parity classes (MODE 2)
inline ConvGeom conv_geom_dgrad(int N, int H, int W, int Cin, int ldx, int Cout, int ldg, int KH, int KW, int stride, int pad,
                                int dil, bool parity) {
  ConvGeom g = {};
  g.N = N; g.H = conv_out_dim(H, KH, stride, pad, dil); g.W = conv_out_dim(W, KW, stride, pad, dil); g.C = Cout; g.ldx = ldg;
  g.OH = H; g.OW = W;
  g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad; g.dil = dil; g.transposed = 1;
  g.sshift = __builtin_ctz((unsigned)stride); g.smask = stride - 1;
  g.nq = KH * KW * Cout / 8;
  g.M = (long long)N * H * W;
  g.Kout = Cin; g.ldw = KH * KW * Cout; g.ldy = ldx;
  if (stride > 1 && stride <= 4 && dil == 1 && parity) {
    // parity classes of the input pixels: (ih + pad) mod stride selects the kh that reach a pixel (ConvGeom::cls); one launch,
    // row tiles class by class; g.nq stays the full tap count (it sizes the tap table), g.M the full row count (tile shape)
    g.transposed = 2;
    for (int ph = 0; ph < stride; ++ph)
      for (int pw = 0; pw < stride; ++pw) {
        ConvGeom::ParityClass &c = g.cls[g.ncls];
        c.kh0 = ph; c.kw0 = pw;
        c.nkh = ph < KH ? (KH - ph + stride - 1) / stride : 0;
        c.nkw = pw < KW ? (KW - pw + stride - 1) / stride : 0;
        if (c.nkh == 0 || c.nkw == 0) c.nkh = c.nkw = 0;
        c.h0 = ((ph - pad) % stride + stride) % stride;
        c.w0 = ((pw - pad) % stride + stride) % stride;
        c.Hc = c.h0 < H ? (H - c.h0 + stride - 1) / stride : 0;
        c.Wc = c.w0 < W ? (W - c.w0 + stride - 1) / stride : 0;
        c.tile0 = 0;
        if (c.Hc > 0 && c.Wc > 0) ++g.ncls;
      }
  }
  return g;
}

// Pixel-range split of a weight gradient (dense and sparse): `steps` 64-pixel steps over `tiles` tiles of dW on `slots` resident
// workgroups.  The launch must fit ONE residency round: every workgroup runs the same number of steps, so a grid of 513
// workgroups on 512 slots takes twice as long as one of 512 (measured: 130 vs 66 us on the 128 -> 128 layer).  Each split costs a
// full fp32 slab of dW, and a workgroup runs at least `min_steps` steps.
struct SplitPlan { int splits; long long rows_per_split; };  // rows_per_split: multiple of 64
inline SplitPlan plan_splits(long long steps, int tiles, int slots, int min_steps) {
  long long want = tiles >= slots ? 1 : slots / tiles;
  if (want > steps / min_steps) want = steps / min_steps;
  if (want < 1) want = 1;
  const long long per = (steps + want - 1) / want;
  return {(int)((steps + per - 1) / per), per * 64};
}

}  // namespace
}  // namespace bfhip
