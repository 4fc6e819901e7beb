// conv2d.hip -- dense 2-D convolution on channels-last (NHWC) bf16 activations as an implicit GEMM on the gfx950 matrix
// cores: forward and data gradient, with BatchNorm statistics accumulated in the forward epilogue (weight gradient: conv2d_wgrad.hip).
//
// Layers served (SURVEY 8 a-8 ... a-11): ConvFuser 336->256 3x3 (BF/bevfusion_head.py:26-38), SECOND's twelve 3x3 convs and
// SECONDFPN's 1x1 conv (mmdet3d/models/backbones/second.py:27-95, necks/second_fpn.py:30-94), the head's shared_conv
// (BF/bevfusion_head.py:95-102), depthnet / downsample of the view transform (BF/depth_lss.py:592-620) and the LSS-FPN
// lateral / fpn convs (BF/bevfusion_necks.py:50-72).  Any kernel size / stride / padding / dilation, groups = 1,
// channel counts that are multiples of 8.
//
// Formulation.  y[m][co] = sum_k A[m][k] * Wt[co][k], m = (n, oh, ow), k = (kh, kw, ci): the weight of a channels-last conv,
// [Cout][KH][KW][Cin], IS the row-major B^T operand; A is never materialised -- each 16-byte piece (8 channels of one tap
// of one pixel) is fetched straight from the activation into LDS by `global_load_lds_dwordx4` with a per-lane source
// address (padding / tails read a zero page).  The data gradient is the same kernel in "transposed" mode (rows = input
// pixels, gathered tensor = dy, oh = (ih + pad - kh*dil) / stride when divisible) over the [Cin][KH][KW][Cout] transpose
// of the weight.
// Tile: 128 rows x (64 | 128) columns per 256-thread workgroup, K step 64 (bf16), 4 waves as 2 x 2, each wave a
// 64 x (32 | 64) block of `v_mfma_f32_32x32x16_bf16` accumulators; two LDS buffers per operand, the next step's loads are
// issued before the current step's MFMAs (one barrier per step).  LDS images are written linearly by the DMA; the bank
// swizzle lives in the SOURCE chunk a lane fetches and in the read address (same involution on both sides).
#include "conv_common.h"

namespace bfhip {
namespace {

// source address of piece (dh, dw, ci) for the row whose bases are (nb, hb, wb); out of range -> zero page.
// Kept short on purpose: it runs once per 16-byte piece (4 + NB times per wave and K step) beside 16 MFMAs -- no integer
// division (transposed strides are powers of two: shift + mask), 32-bit element offsets (tensors < 2^31 elements).
template <bool TR>
__device__ __forceinline__ const bf16_t *piece_src(const bf16_t *x, const ConvGeom &g, bool row_ok, int nb, int hb, int wb,
                                                   unsigned info, const bf16_t *zsrc) {
  const int dh = info >> 24, dw = (info >> 16) & 0xff, ci = info & 0xffff;
  int ih, iw;
  bool ok = row_ok;
  if (!TR) {
    ih = hb + dh;
    iw = wb + dw;
  } else {
    const int th = hb - dh, tw = wb - dw;
    ok = ok && ((th | tw) >= 0) && (((th | tw) & g.smask) == 0);
    ih = th >> g.sshift;
    iw = tw >> g.sshift;
  }
  ok = ok && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
  const unsigned off = (unsigned)(nb + ih * g.W + iw) * (unsigned)g.ldx + (unsigned)ci;
  return ok ? x + off : zsrc;
}

// ---- epilogue of the implicit-GEMM kernel: (optional) BatchNorm statistics of the raw accumulators, then
// accumulators -> LDS [BM][BN] -> 16-byte coalesced stores.  M rows, Kout columns, row pitch ldy.
// RowMap: GEMM row -> output pixel index (identity except for the parity-class data gradient)
struct RowIdentity {
  __device__ __forceinline__ long long operator()(long long m) const { return m; }
};
struct RowParityClass {
  int Hc, Wc, H, W, h0, w0, stride;
  __device__ __forceinline__ long long operator()(long long m) const {
    // 32-bit arithmetic: every entry point requires N * H * W * pitch < 2^31 (a 64-bit division is ~5x the instructions, and
    // this runs once per 16-byte store)
    const unsigned mu = (unsigned)m, hw = (unsigned)(Hc * Wc);
    const unsigned n = mu / hw, rem = mu - n * hw;
    const unsigned i = rem / (unsigned)Wc, j = rem - i * (unsigned)Wc;
    return (long long)((n * (unsigned)H + h0 + i * stride) * (unsigned)W + w0 + j * stride);
  }
};

// A second gradient path into the tensor the epilogue writes (residual connections): bf16, dense (pixel pitch `ld`), on the
// output's own pixel grid (sub == 1) or on the grid of its even pixels [N, ceil(H/2), ceil(W/2)] (sub == 2: the gradient of a
// stride-2 1x1 shortcut, which only reaches the pixels with even h and w)
struct Addend {
  const bf16_t *p;
  int sub, ld, H, W;
};

template <int WGM, int WGN, int MI, int NI, bool OUT_F32, typename RowMap = RowIdentity>
__device__ __forceinline__ void igemm_epilogue(f32x16 (&acc)[MI][NI], unsigned char *smem, int tm, long long m0, int n0,
                                               long long M, int Kout, int ldy, const float *__restrict__ bias,
                                               void *__restrict__ y, float *__restrict__ stat_partial,
                                               RowMap row_map = RowMap(), Addend add = Addend{nullptr, 0, 0, 0, 0}) {
  constexpr int NTHREADS = WGM * WGN * 64;
  constexpr int BN = WGN * NI * 32, BM = WGM * MI * 32;
  constexpr int PR = BM / 128;   // statistics partial rows of this tile (one per 128 pixels)
  constexpr int G = WGM / PR;    // wave rows that make up one partial row
  static_assert(BM % 128 == 0 && G * PR == WGM, "tile rows must be whole 128-row statistic groups");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w / WGN, wn = w % WGN;
  const int l31 = lane & 31, lh = lane >> 5;
  __syncthreads();  // every wave is done with the staging buffers: reuse them for the epilogue

  // ---- BatchNorm statistics of the raw accumulators (rows beyond M are exact zeros): per-column sum / sum of squares,
  //      one partial row per 128 rows of the tile
  if (stat_partial) {
    float *sred = (float *)(smem);  // [WGM][BN][2]
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float s = 0.f, s2 = 0.f;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) { float v = acc[mi][ni][r]; s += v; s2 += v * v; }
      s += __shfl_xor(s, 32);
      s2 += __shfl_xor(s2, 32);
      if (lh == 0) {
        int col = wn * (NI * 32) + ni * 32 + l31;
        sred[(wm * BN + col) * 2 + 0] = s;
        sred[(wm * BN + col) * 2 + 1] = s2;
      }
    }
    __syncthreads();
    const int total_rows = (int)((M + 127) / 128);
    for (int e = tid; e < PR * BN; e += NTHREADS) {
      const int pr = e / BN, col = e - pr * BN;
      const int prow = tm * PR + pr;
      if (n0 + col < Kout && prow < total_rows) {
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int gi = 0; gi < G; ++gi) {
          const float *q = sred + ((pr * G + gi) * BN + col) * 2;
          t0 += q[0];
          t1 += q[1];
        }
        stat_partial[((size_t)prow * 2 + 0) * Kout + n0 + col] = t0;
        stat_partial[((size_t)prow * 2 + 1) * Kout + n0 + col] = t1;
      }
    }
    __syncthreads();
  }

  // ---- output: accumulators -> LDS [BM][BN] (row-major) -> 16-byte coalesced stores
  constexpr int ESZ = OUT_F32 ? 4 : 2;
  constexpr int ROWB = BN * ESZ;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int col = wn * (NI * 32) + ni * 32 + l31;
    const float bv = (bias && n0 + col < Kout) ? bias[n0 + col] : 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * (MI * 32) + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float v = acc[mi][ni][r] + bv;
        if (OUT_F32) *(float *)(smem + row * ROWB + col * 4) = v;
        else *(bf16_t *)(smem + row * ROWB + col * 2) = (bf16_t)bf16_rne(v);
      }
  }
  __syncthreads();
  constexpr int CPR = ROWB / 16;  // 16-byte pieces per row
  constexpr int EPC = 16 / ESZ;   // elements per piece
  for (int idx = tid; idx < BM * CPR; idx += NTHREADS) {
    const int row = idx / CPR, c = idx - row * CPR;
    const long long m = m0 + row;
    const int col = n0 + c * EPC;
    if (m >= M || col >= Kout) continue;
    unsigned char *dst = (unsigned char *)y + ((size_t)row_map(m) * ldy + col) * ESZ;
    const unsigned char *src = smem + row * ROWB + c * 16;
    const bf16_t *rs = nullptr;
    if (!OUT_F32 && add.p) {
      if (add.sub == 2) {  // addend on the even-pixel grid: rows with odd h or w receive nothing from it
        const unsigned mu = (unsigned)row_map(m), hw = (unsigned)(add.H * add.W);
        const unsigned n = mu / hw, rem = mu - n * hw;
        const unsigned h = rem / (unsigned)add.W, w = rem - h * (unsigned)add.W;
        if (((h | w) & 1u) == 0)
          rs = add.p + ((size_t)((n * (unsigned)((add.H + 1) >> 1) + (h >> 1)) * (unsigned)((add.W + 1) >> 1) + (w >> 1)) * add.ld + col);
      } else {
        rs = add.p + ((size_t)row_map(m) * add.ld + col);
      }
    }
    if (rs) {
      // bf16 output + bf16 addend (the other gradient path into the same tensor): widened, added to the already rounded
      // result in fp32, rounded once more -- what a separate bf16 add kernel computes
      bf16_t *d16 = (bf16_t *)dst;
      const bf16_t *s16 = (const bf16_t *)src;
      if (col + EPC <= Kout && ((((uintptr_t)dst) | ((uintptr_t)rs)) & 15) == 0) {
        const uint4 a4 = *(const uint4 *)src, b4 = *(const uint4 *)rs;
        const unsigned a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
        unsigned o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float lo = __uint_as_float(a[q] << 16) + __uint_as_float(b[q] << 16);
          const float hi = __uint_as_float(a[q] & 0xffff0000u) + __uint_as_float(b[q] & 0xffff0000u);
          o[q] = bf16_rne(lo) | (bf16_rne(hi) << 16);
        }
        *(uint4 *)dst = make_uint4(o[0], o[1], o[2], o[3]);
        continue;
      }
      for (int e = 0; e < EPC && col + e < Kout; e += 2) {
        if (col + e + 1 < Kout && ((((uintptr_t)(d16 + e)) | ((uintptr_t)(rs + e))) & 3) == 0) {
          const unsigned a = *(const unsigned *)(s16 + e), b = *(const unsigned *)(rs + e);
          const float lo = __uint_as_float(a << 16) + __uint_as_float(b << 16);
          const float hi = __uint_as_float(a & 0xffff0000u) + __uint_as_float(b & 0xffff0000u);
          *(unsigned *)(d16 + e) = bf16_rne(lo) | (bf16_rne(hi) << 16);
        } else {
          for (int q = e; q < e + 2 && col + q < Kout; ++q)
            d16[q] = (bf16_t)bf16_rne(__uint_as_float((unsigned)s16[q] << 16) + __uint_as_float((unsigned)rs[q] << 16));
        }
      }
      continue;
    }
    if (col + EPC <= Kout && (((uintptr_t)dst) & 15) == 0) *(uint4 *)dst = *(const uint4 *)src;
    else
      for (int e = 0; e < EPC && col + e < Kout; ++e) {
        if (OUT_F32) ((float *)dst)[e] = ((const float *)src)[e];
        else ((bf16_t *)dst)[e] = ((const bf16_t *)src)[e];
      }
  }
}

// ------------------------------------------------------------------------------------------------ forward / dgrad
// Tile BM = WGM*MI*32 rows x BN = WGN*NI*32 columns, WGM x WGN waves with (MI*32) x (NI*32) wave tiles of 32x32x16 MFMAs, a
// ring of STAGES LDS stages of one K step (64 bf16) each.  Rows are 128 bytes (8 pieces); piece c of row r sits at position
// c ^ ((r >> 1) & 7): the 16 rows a ds_read_b128 lane group touches land on 16 distinct 16-byte slots.
//   <2, 2, 2, NI, 2>: 128 x (64 | 128) tiles, 256 threads, two stages, two workgroups per CU (small problems, narrow outputs)
//   <2, 4, 4, 2, 2> : 256 x 256 tiles, 512 threads (8 waves as 2 x 4, wave tile 128 x 64), two stages of 64 KB: half the
//                     operand bytes per flop of the 128 x 128 tile (the L2 -> LDS fill rate of a CU, ~40-70 GB/s, is what the
//                     small tile runs into) and 3/4 of its LDS fragment reads per MFMA; for wide outputs with enough tiles
//   (<4, 2, 2, 2, 3>, 256 x 128 tiles with 64 x 64 wave tiles and a three-stage ring, measured no gain and is no longer built)
// MODE 0: forward gather; 1: data gradient (transposed gather over all taps, rows = all input pixels); 2: data gradient of a
// strided convolution, one parity class of input pixels per launch: a pixel (ih, iw) is reached only by the taps with
// kh = (ih + pad) mod stride (mod stride), so the class walks KH*KW / stride^2 of the taps instead of meeting holes at the rest
//   <2, 2, 2, NI, 1>: ONE stage, at most 128 registers, four workgroups per CU (the pointwise kernel's recipe with the tap
//                     gather): nothing overlaps inside a workgroup, residency hides the latency -- for the small maps of the
//                     ResNet-50 trunk, where tiles are few and K loops short (BFHIP_CONV_SINGLE_STAGE)
template <int WGM, int WGN, int MI, int NI, int STAGES, bool OUT_F32, int MODE>
__global__ __launch_bounds__(WGM * WGN * 64, (STAGES == 1 ? 4 : (WGM * WGN > 4 ? 1 : 2))) void conv_igemm_kernel(
    const bf16_t *__restrict__ x, const bf16_t *__restrict__ wt, const float *__restrict__ bias, void *__restrict__ y,
    float *__restrict__ stat_partial, ConvGeom g, int tiles_m, int tiles_n) {
  constexpr bool TR = MODE != 0;
  constexpr int NWAVES = WGM * WGN, NTHREADS = NWAVES * 64;
  constexpr int BN = WGN * NI * 32, BM = WGM * MI * 32, BK = 64;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, S_BYTES = A_BYTES + B_BYTES;
  constexpr int NA = (BM / 8) / NWAVES;  // A DMA instructions per wave and stage (8 rows each)
  constexpr int NB = (BN / 8) / NWAVES;  // B DMA instructions per wave and stage
  constexpr int GL = NA + NB;            // DMA instructions per wave and stage
  static_assert(NA >= 1 && NA * 8 * NWAVES == BM && NB >= 1 && NB * 8 * NWAVES == BN, "tiles must split into whole DMA instructions");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  unsigned *taps = (unsigned *)(smem + STAGES * S_BYTES);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long lb = xcd_chunked_block(blockIdx.x, (long long)tiles_m * tiles_n);
  const int tn = (int)(lb % tiles_n);
  int tm = (int)(lb / tiles_n);
  long long M = g.M;  // GEMM rows and K pieces of this workgroup's problem (MODE 2: of its parity class)
  int nq = g.nq;
  ConvGeom::ParityClass pc = {};
  if (MODE == 2) {
    int c = 0;
    while (c + 1 < g.ncls && tm >= g.cls[c + 1].tile0) ++c;
    pc = g.cls[c];
    tm -= pc.tile0;
    M = (long long)g.N * pc.Hc * pc.Wc;
    nq = pc.nkh * pc.nkw * (g.C >> 3);
  }
  const long long m0 = (long long)tm * BM;
  const int n0 = tn * BN;

  if (MODE == 2 && nq == 0) {
    // no tap reaches this parity class (e.g. three of the four classes of a 1x1 stride-2 layer): its gradient is zero -- plain
    // 16-byte zero stores, no staging, no accumulators
    constexpr int ESZ = OUT_F32 ? 4 : 2, EPC = 16 / ESZ, CPR = BN / EPC;
    const RowParityClass rm{pc.Hc, pc.Wc, g.OH, g.OW, pc.h0, pc.w0, g.stride};
    for (int idx = tid; idx < BM * CPR; idx += NTHREADS) {
      const int row = idx / CPR, c = idx - row * CPR;
      const long long m = m0 + row;
      const int col = n0 + c * EPC;
      if (m >= M || col >= g.Kout) continue;
      unsigned char *dst = (unsigned char *)y + ((size_t)rm(m) * g.ldy + col) * ESZ;
      if (col + EPC <= g.Kout && (((uintptr_t)dst) & 15) == 0) *(uint4 *)dst = make_uint4(0u, 0u, 0u, 0u);
      else
        for (int e = 0; e < EPC && col + e < g.Kout; ++e) {
          if (OUT_F32) ((float *)dst)[e] = 0.f;
          else ((bf16_t *)dst)[e] = 0;
        }
    }
    return;
  }

  for (int q = tid; q < nq; q += NTHREADS) {
    int k = q * 8;
    int tap = k / g.C, ci = k - tap * g.C;
    int kh, kw;
    if (MODE == 2) {  // the class's taps only (dilation 1)
      const int a = tap / pc.nkw;
      kh = pc.kh0 + a * g.stride;
      kw = pc.kw0 + (tap - a * pc.nkw) * g.stride;
    } else {
      kh = tap / g.KW;
      kw = tap - kh * g.KW;
    }
    taps[q] = ((unsigned)(kh * g.dil) << 24) | ((unsigned)(kw * g.dil) << 16) | (unsigned)ci;
  }

  // ---- per-lane staging state: NA A rows (one per DMA instruction) and NB B rows; every wave stages NA*8 A rows
  const int lrow = lane >> 3, lpos = lane & 7;
  int nb[NA], hb[NA], wb[NA];
  bool rok[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    long long m = m0 + w * (NA * 8) + i * 8 + lrow;
    rok[i] = m < M;
    long long mm = rok[i] ? m : 0;
    int n, oh, ow;
    const unsigned mu = (unsigned)mm;  // rows < 2^31 (entry-point precondition): 32-bit divisions
    if (MODE == 2) {
      const unsigned hw = (unsigned)(pc.Hc * pc.Wc);
      const unsigned nn = mu / hw, rem = mu - nn * hw;
      const unsigned ci_ = rem / (unsigned)pc.Wc;
      n = (int)nn;
      oh = pc.h0 + (int)ci_ * g.stride;
      ow = pc.w0 + (int)(rem - ci_ * (unsigned)pc.Wc) * g.stride;
    } else {
      const unsigned hw = (unsigned)(g.OH * g.OW);
      const unsigned nn = mu / hw, rem = mu - nn * hw;
      n = (int)nn;
      oh = (int)(rem / (unsigned)g.OW);
      ow = (int)(rem - (unsigned)oh * (unsigned)g.OW);
    }
    nb[i] = n * g.H * g.W;
    hb[i] = TR ? oh + g.pad : oh * g.stride - g.pad;
    wb[i] = TR ? ow + g.pad : ow * g.stride - g.pad;
  }
  const bf16_t *wrow[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    int co = n0 + w * (NB * 8) + i * 8 + lrow;
    wrow[i] = co < g.Kout ? wt + (size_t)co * g.ldw : nullptr;
  }
  __syncthreads();  // tap table ready

  const int nt = (nq + 7) >> 3;
  const bf16_t *zsrc = zero_src();
  auto stage = [&](int t, int buf) {  // exactly GL DMA instructions per wave (the counted waits rely on it)
    unsigned char *dA = smem + buf * S_BYTES + (w * (NA * 8)) * 128;
    unsigned char *dB = smem + buf * S_BYTES + A_BYTES + (w * (NB * 8)) * 128;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int swz = ((w * (NA * 8) + i * 8 + lrow) >> 1) & 7;
      const int q = t * 8 + (lpos ^ swz);
      const bf16_t *src = q < nq ? piece_src<TR>(x, g, rok[i], nb[i], hb[i], wb[i], taps[q], zsrc) : zsrc;
      glds16(src, dA + i * 1024);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int swz = ((w * (NB * 8) + i * 8 + lrow) >> 1) & 7;
      const int q = t * 8 + (lpos ^ swz);
      const bf16_t *src = zsrc;
      if (wrow[i] && q < nq) {
        if (MODE == 2) {  // the weight row holds all taps: this piece's tap is (dh, dw) of the table entry
          const unsigned info = taps[q];
          src = wrow[i] + ((size_t)((info >> 24) * g.KW + ((info >> 16) & 0xff)) * g.C + (info & 0xffff));
        } else {
          src = wrow[i] + (size_t)q * 8;
        }
      }
      glds16(src, dB + i * 1024);
    }
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int wm = w / WGN, wn = w % WGN;
  const int l31 = lane & 31, lh = lane >> 5, rswz = (lane >> 1) & 7;  // ((row >> 1) & 7) of row = 32*j + l31
  const int aoff = (wm * (MI * 32) + l31) * 128, boff = A_BYTES + (wn * (NI * 32) + l31) * 128;

#pragma unroll
  for (int s0 = 0; s0 < STAGES - 1; ++s0)
    if (s0 < nt) stage(s0, s0);
  int buf = 0, nbuf = STAGES - 1;  // stage holding step t / stage the next DMA goes to
  for (int t = 0; t < nt; ++t) {
    if (STAGES == 1) {
      if (t) __syncthreads();  // every wave has consumed step t - 1
      stage(t, 0);
    }
    // step t must have landed; the DMA of the (up to STAGES - 2) later steps stays in flight
    if (STAGES <= 2 || nt - 1 - t == 0) wait_vmcnt<0>();
    else if (STAGES == 3 || nt - 1 - t == 1) wait_vmcnt<GL>();
    else wait_vmcnt<2 * GL>();
    __builtin_amdgcn_s_barrier();  // all of step t is in LDS; every wave is done reading step t - 1
    const unsigned char *pA = smem + buf * S_BYTES + aoff, *pB = smem + buf * S_BYTES + boff;
    if (STAGES > 1 && t + STAGES - 1 < nt) stage(t + STAGES - 1, nbuf);  // before the MFMAs: issuing it after the first K quarter's
                                                           // MFMAs (address generation in their shadow) measured 5-10 % slower
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int pos = ((2 * ks + lh) ^ rswz) << 4;
      bf16x8 a[MI], b[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi] = *(const bf16x8 *)(pA + mi * 32 * 128 + pos);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) b[ni] = *(const bf16x8 *)(pB + ni * 32 * 128 + pos);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    buf = buf + 1 == STAGES ? 0 : buf + 1;
    nbuf = nbuf + 1 == STAGES ? 0 : nbuf + 1;
  }
  if (MODE == 2)
    igemm_epilogue<WGM, WGN, MI, NI, OUT_F32, RowParityClass>(acc, smem, tm, m0, n0, M, g.Kout, g.ldy, bias, y, stat_partial,
                                                              RowParityClass{pc.Hc, pc.Wc, g.OH, g.OW, pc.h0, pc.w0, g.stride});
  else
    igemm_epilogue<WGM, WGN, MI, NI, OUT_F32>(acc, smem, tm, m0, n0, M, g.Kout, g.ldy, bias, y, stat_partial);
}

// ------------------------------------------------------------------------------------------------ pointwise (1x1, stride 1)
// y[m][co] = sum_ci x[m][ci] * Wt[co][ci]: a plain GEMM over a tall activation matrix with a short K (64 ... 256 in the
// ResNet-50 trunk's bottlenecks, where M = 270 k rows): one to four K steps per tile, so a ring of stages has nothing to
// overlap inside a workgroup and the layer is bound by HBM, not by the matrix cores.  What hides the latency here is
// residency: ONE stage of one K step (32 KB for a 128 x 128 tile), at most 128 registers, four to five workgroups per CU
// at different points of load -> MFMA -> epilogue; no tap table, no divisions (row m IS pixel m).  Same tile, LDS image,
// swizzle and epilogue (BatchNorm statistics, LDS transpose, 16-byte stores) as conv_igemm_kernel<2, 2, 2, NI>.
// DIR (0 forward, 1 data gradient) only names the instantiation, so that a kernel trace tells the two uses apart.
template <int NI, bool OUT_F32, int DIR>
__global__ __launch_bounds__(256, 4) void conv_pw_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ wt,
                                                         const float *__restrict__ bias, void *__restrict__ y,
                                                         float *__restrict__ stat_partial, long long M, int C, int ldx, int Kout,
                                                         int ldw, int ldy, int tiles_m, int tiles_n, Addend add) {
  constexpr int WGN = 2, MI = 2;
  constexpr int BM = 128, BN = NI * 64;
  constexpr int A_BYTES = BM * 128;
  constexpr int NA = 4, NB = BN / 32;  // DMA instructions per wave and K step (8 rows of 128 bytes each)
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long lb = xcd_chunked_block(blockIdx.x, (long long)tiles_m * tiles_n);
  const int tn = (int)(lb % tiles_n), tm = (int)(lb / tiles_n);
  const long long m0 = (long long)tm * BM;
  const int n0 = tn * BN;
  const int nq = C >> 3, nt = (nq + 7) >> 3;
  const int lrow = lane >> 3, lpos = lane & 7;
  const bf16_t *zsrc = zero_src();
  const bf16_t *arow[NA], *brow[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const long long m = m0 + w * 32 + i * 8 + lrow;
    arow[i] = m < M ? x + (unsigned)m * (unsigned)ldx : nullptr;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int co = n0 + w * (NB * 8) + i * 8 + lrow;
    brow[i] = co < Kout ? wt + (size_t)co * ldw : nullptr;
  }
  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
  const int wm = w / WGN, wn = w % WGN;
  const int l31 = lane & 31, lh = lane >> 5, rswz = (lane >> 1) & 7;
  const unsigned char *pA = smem + (wm * 64 + l31) * 128, *pB = smem + A_BYTES + (wn * (NI * 32) + l31) * 128;
  unsigned char *dA = smem + (w * 32) * 128, *dB = smem + A_BYTES + (w * (NB * 8)) * 128;
  for (int t = 0; t < nt; ++t) {
    if (t) __syncthreads();  // every wave has consumed the previous K step
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int q = t * 8 + (lpos ^ (((w * 32 + i * 8 + lrow) >> 1) & 7));
      glds16(arow[i] && q < nq ? arow[i] + q * 8 : zsrc, dA + i * 1024);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int q = t * 8 + (lpos ^ (((w * (NB * 8) + i * 8 + lrow) >> 1) & 7));
      glds16(brow[i] && q < nq ? brow[i] + q * 8 : zsrc, dB + i * 1024);
    }
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int pos = ((2 * ks + lh) ^ rswz) << 4;
      bf16x8 a[MI], b[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi] = *(const bf16x8 *)(pA + mi * 32 * 128 + pos);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) b[ni] = *(const bf16x8 *)(pB + ni * 32 * 128 + pos);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
  }
  igemm_epilogue<2, WGN, MI, NI, OUT_F32>(acc, smem, tm, m0, n0, M, Kout, ldy, bias, y, stat_partial, RowIdentity(), add);
}

// Wt'[ci][kh][kw][co] = W[co][kh][kw][ci]  (the dgrad's B^T operand)
__global__ __launch_bounds__(256) void conv_weight_transpose_kernel(const bf16_t *__restrict__ w, bf16_t *__restrict__ wt,
                                                                    int Cout, int taps, int Cin) {
  __shared__ bf16_t tile[32][33];
  const int tap = blockIdx.z, c0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    int co = o0 + r, ci = c0 + tx;
    tile[r][tx] = (co < Cout && ci < Cin) ? w[((size_t)co * taps + tap) * Cin + ci] : (bf16_t)0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    int ci = c0 + r, co = o0 + tx;
    if (ci < Cin && co < Cout) wt[((size_t)ci * taps + tap) * Cout + co] = tile[tx][r];
  }
}

// The same for a table of weights in ONE launch (all layers of a model after the optimizer step: a training step otherwise
// pays one ~5 us transpose launch per data gradient, 69 per step).  Segment i owns blocks [blk0[i], blk0[i + 1]).
struct WtSeg {
  const void *src;   // [Cout][taps][Cin], bf16 or fp32 (src_f32)
  bf16_t *dst;       // [Cin][taps][Cout]
  int Cout, taps, Cin, src_f32;
  long long blk0;
};
__global__ __launch_bounds__(256) void conv_weight_transpose_batched_kernel(const WtSeg *__restrict__ segs, int nseg) {
  __shared__ bf16_t tile[32][33];
  const long long b = blockIdx.x;
  int lo = 0, hi = nseg - 1;  // largest segment with blk0 <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].blk0 <= b) lo = mid; else hi = mid - 1;
  }
  const WtSeg sg = segs[lo];
  const int nx = (sg.Cin + 31) >> 5, ny = (sg.Cout + 31) >> 5;
  int local = (int)(b - sg.blk0);
  const int bx = local % nx; local /= nx;
  const int by = local % ny;
  const int tap = local / ny;
  if (tap >= sg.taps) return;
  const int c0 = bx * 32, o0 = by * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int co = o0 + r, ci = c0 + tx;
    bf16_t v = 0;
    if (co < sg.Cout && ci < sg.Cin) {
      const size_t i = ((size_t)co * sg.taps + tap) * sg.Cin + ci;
      v = sg.src_f32 ? (bf16_t)bf16_rne(((const float *)sg.src)[i]) : ((const bf16_t *)sg.src)[i];
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int ci = c0 + r, co = o0 + tx;
    if (ci < sg.Cin && co < sg.Cout) sg.dst[((size_t)ci * sg.taps + tap) * sg.Cout + co] = tile[tx][r];
  }
}

// fp32 operand -> bf16 pair (hi = bf16(v), lo = bf16(v - hi)), written in the two layouts the three-product fp32 convolution
// consumes (conv2d.py: _Conv2dSplitFunction): channel blocks [P][3C] and batch blocks [3][P][C]; bit k of an order word says
// whether block k holds hi (0) or lo (1).  One thread = 8 channels of one pixel.
__global__ __launch_bounds__(256) void split_bf16x3_kernel(const float *__restrict__ src, long long P, int C, bf16_t *__restrict__ chan,
                                                           int order_chan, bf16_t *__restrict__ batch, int order_batch) {
  const int cv = C >> 3;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P * cv) return;
  const long long p = t / cv;
  const int c = (int)(t - p * cv) << 3;
  const float4 a = *(const float4 *)(src + p * C + c), b = *(const float4 *)(src + p * C + c + 4);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  unsigned hi[8], lo[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    hi[j] = bf16_rne(v[j]);
    lo[j] = bf16_rne(v[j] - __uint_as_float(hi[j] << 16));
  }
  const uint4 H4 = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
  const uint4 L4 = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (chan) *(uint4 *)(chan + p * (3LL * C) + (long long)k * C + c) = ((order_chan >> k) & 1) ? L4 : H4;
    if (batch) *(uint4 *)(batch + ((long long)k * P + p) * C + c) = ((order_batch >> k) & 1) ? L4 : H4;
  }
}

// ------------------------------------------------------------------------------------------------ host side
// 1x1, stride 1, no padding (forward, or the data gradient of such a layer: both are plain GEMMs over the pixel matrix) with a
// short K: conv_pw_kernel.  BFHIP_CONV_PW_MAXC: largest channel count of the gathered tensor it takes (0 = never)
bool takes_pointwise(const ConvGeom &g) {
  static const int max_c = env_int("BFHIP_CONV_PW_MAXC", 4096);
  return g.KH == 1 && g.KW == 1 && g.stride == 1 && g.pad == 0 && g.transposed != 2 && g.C <= max_c;
}

// tile shapes (see conv_igemm_kernel): 0 = 128 x 64, 1 = 128 x 128, 2 = 256 x 256 (bf16 output, wide GEMMs with at least
// ~1.5 tiles per CU); pointwise: conv_pw_kernel on 128 x BN tiles, one stage
struct IgemmChoice {
  bool pointwise;
  int shape, stages, BM, BN, tiles_m, tiles_n;  // grid = tiles_m * tiles_n
  size_t lds;                                   // dynamic LDS bytes
  int tile0[17];  // parity-class data gradient: first row tile of class c, tile0[ncls] = tiles_m (ConvGeom::cls[].tile0)
};

// The decision, free of launches: a function of the geometry, the output type, the knobs and the CU count of the device
// (`cus`; the residency figures below are per CU: two 128 x 128 workgroups, three 128 x 64 or single-stage ones).
IgemmChoice choose_igemm(const ConvGeom &g, int out_f32, int cus) {
  IgemmChoice c = {};
  if (takes_pointwise(g)) {
    c.pointwise = true;
    c.stages = 1; c.BM = 128; c.BN = g.Kout > 64 ? 128 : 64;
    c.tiles_m = ceil_div(g.M, 128);
    c.tiles_n = ceil_div(g.Kout, c.BN);
    const size_t stage = (size_t)(128 + c.BN) * 128, epi = (size_t)128 * c.BN * (out_f32 ? 4 : 2);
    c.lds = stage > epi ? stage : epi;
    return c;
  }
  // BFHIP_CONV_TILE256: 0 = never, 1 = by the rule below, 2 = whenever the output is bf16 and wider than 128 (tests)
  static const int tile256 = env_int("BFHIP_CONV_TILE256", 1);
  static const int tile256_min = env_int("BFHIP_CONV_TILE256_MIN", 384);
  int shape = g.Kout > 64 ? 1 : 0;
  const long long t256 = (long long)ceil_div(g.M, 256) * ceil_div(g.Kout, 256);
  // enough tiles for the 256 one-workgroup CUs, and at most 1/8 of the 256-wide column tiles wasted
  const bool fits256 = t256 >= tile256_min && (long long)ceil_div(g.Kout, 256) * 256 * 8 <= (long long)g.Kout * 9;
  if (tile256 && !out_f32 && g.Kout > 128 && (fits256 || tile256 == 2)) shape = 2;
  static const int quant = env_int("BFHIP_CONV_QUANT", 1);
  if (quant && shape == 1) {
    // 128 x 128 tiles run two workgroups per CU: a tile count just above a whole number of rounds leaves the last round almost
    // empty; 128 x 64 tiles (three per CU) quantise finer (depthnet / LSS-FPN 3x3 on the 24 x 32 x 88 maps, 1 056 tiles = 2.06
    // rounds: forward 0.167 -> 0.161 ms, backward 0.344 -> 0.318 ms)
    const long long t = (long long)ceil_div(g.M, 128) * ceil_div(g.Kout, 128);
    const double rounds = (double)t / (2.0 * cus);
    if (rounds > 1.0 && rounds < 4.0 && rounds - (long long)rounds < 0.15) shape = 0;
  }
  // less than half a residency round of 128 x 128 tiles (small maps with long K: ResNet layer4's 3x3 layers are 132 tiles of 72 K
  // steps): 128 x 64 tiles double the workgroups; BFHIP_CONV_SMALL_GRID=0 switches the rule off
  static const int small_grid = env_int("BFHIP_CONV_SMALL_GRID", 1);
  if (small_grid && shape == 1 && g.transposed != 2 && (long long)ceil_div(g.M, 128) * ceil_div(g.Kout, 128) < cus) shape = 0;
  // One stage + four workgroups per CU for the 128-row tiles (BFHIP_CONV_SINGLE_STAGE: 0 never, 1 by rule, 2 always).  Residency
  // hides the load latency when there are enough workgroups to fill it (>= 3 per CU) or the K loop is too short for a ring to reach
  // steady state (<= 18 steps; the parity classes of a strided data gradient: 1/4 ... 1/stride^2 of the taps each); few tiles
  // with a long K loop keep the two-stage ring.  Measured, same box (tools/resnet_conv_micro.py / conv_micro.py, us, two-stage ->
  // one stage): ResNet 3x3 64 ch fwd 48.5 -> 42.8, dgrad 51.6 -> 44.9; 128 ch 44.9 -> 39.5, 52.2 -> 43.8; stride-2 data gradients
  // 93.5 -> 72.7, 82.2 -> 69.9, 88.1 -> 74.9; SECOND 128 -> 128 fwd 63.6 -> 55.1; shared_conv 198.5 -> 184.9; downsample 80 -> 80
  // 151.8 -> 128.6; against that 256 ch on 16 x 44 maps (264 tiles, 36 steps) 47.6 -> 52.7 and 512 ch on 8 x 22 66.0 -> 84.4
  static const int single = env_int("BFHIP_CONV_SINGLE_STAGE", 1);
  const long long tiles128 = (long long)ceil_div(g.M, 128) * ceil_div(g.Kout, shape == 0 ? 64 : 128);
  const bool one_stage = shape <= 1 && single && (single == 2 || g.transposed == 2 || tiles128 >= 3LL * cus || (g.nq + 7) / 8 <= 18);
  c.shape = shape; c.stages = one_stage ? 1 : 2;
  c.BM = shape == 2 ? 256 : 128; c.BN = shape == 2 ? 256 : (shape == 0 ? 64 : 128);
  c.tiles_m = ceil_div(g.M, c.BM);
  c.tiles_n = ceil_div(g.Kout, c.BN);
  if (g.transposed == 2) {  // row tiles class by class
    c.tiles_m = 0;
    for (int k = 0; k < g.ncls; ++k) {
      c.tile0[k] = c.tiles_m;
      c.tiles_m += ceil_div((long long)g.N * g.cls[k].Hc * g.cls[k].Wc, c.BM);
    }
    c.tile0[g.ncls] = c.tiles_m;
  }
  c.lds = (size_t)c.stages * (c.BM + c.BN) * 128 + (size_t)g.nq * 4;  // stages + tap table
  if (c.stages == 1) {  // the epilogue stages the output tile in the same LDS: BM x BN elements
    const size_t epi = (size_t)c.BM * c.BN * (out_f32 ? 4 : 2);
    if (c.lds < epi) c.lds = epi;
  }
  return c;
}

// ---- the launch of a choice: one instantiation per (tile, stages, output type, direction / gather mode)
struct IgemmArgs { const bf16_t *x, *wt; const float *bias; void *y; float *stat_partial; ConvGeom g; hipStream_t s; Addend add; };

template <int NI, bool F32, int DIR>
void launch_pw(const IgemmArgs &a, const IgemmChoice &c) {
  launch_big_lds<conv_pw_kernel<NI, F32, DIR>>(64 * 1024, dim3((unsigned)((long long)c.tiles_m * c.tiles_n)), dim3(256), c.lds, a.s, a.x, a.wt,
                                               a.bias, a.y, a.stat_partial, a.g.M, a.g.C, a.g.ldx, a.g.Kout, a.g.ldw, a.g.ldy, c.tiles_m, c.tiles_n, a.add);
}
template <int NI, bool F32>
void launch_pw(const IgemmArgs &a, const IgemmChoice &c) { a.g.transposed ? launch_pw<NI, F32, 1>(a, c) : launch_pw<NI, F32, 0>(a, c); }

template <int WGM, int WGN, int MI, int NI, int ST, bool F32, int MODE>
void launch_ig(const IgemmArgs &a, const IgemmChoice &c) {
  launch_big_lds<conv_igemm_kernel<WGM, WGN, MI, NI, ST, F32, MODE>>(
      (WGM * WGN > 4) ? 159 * 1024 : 80 * 1024, dim3((unsigned)((long long)c.tiles_m * c.tiles_n)), dim3(WGM * WGN * 64), c.lds, a.s, a.x, a.wt,
      a.bias, a.y, a.stat_partial, a.g, c.tiles_m, c.tiles_n);
}
template <int WGM, int WGN, int MI, int NI, int ST, bool F32>
void launch_ig(const IgemmArgs &a, const IgemmChoice &c) {
  const int m = a.g.transposed;
  m == 2 ? launch_ig<WGM, WGN, MI, NI, ST, F32, 2>(a, c) : m ? launch_ig<WGM, WGN, MI, NI, ST, F32, 1>(a, c) : launch_ig<WGM, WGN, MI, NI, ST, F32, 0>(a, c);
}
template <int NI, int ST>  // the 128-row tiles
void launch_ig128(const IgemmArgs &a, const IgemmChoice &c, int f32) { f32 ? launch_ig<2, 2, 2, NI, ST, true>(a, c) : launch_ig<2, 2, 2, NI, ST, false>(a, c); }

int launch_igemm(const void *x, const void *wt, const float *bias, void *y, float *stat_partial, const ConvGeom &g, int out_f32,
                 hipStream_t s, const char *what, Addend add = Addend{nullptr, 0, 0, 0, 0}) {
  BFHIP_REQUIRE(!add.p || (takes_pointwise(g) && !out_f32),
                "%s: an addend is only fused into the pointwise kernel (1x1, stride 1, no padding, bf16 output)", what);
  const IgemmChoice c = choose_igemm(g, out_f32, device_cus());
  IgemmArgs a = {(const bf16_t *)x, (const bf16_t *)wt, bias, y, stat_partial, g, s, add};
  for (int k = 0; g.transposed == 2 && k <= g.ncls; ++k) a.g.cls[k].tile0 = c.tile0[k];
  if (c.pointwise && c.BN == 128) out_f32 ? launch_pw<2, true>(a, c) : launch_pw<2, false>(a, c);
  else if (c.pointwise) out_f32 ? launch_pw<1, true>(a, c) : launch_pw<1, false>(a, c);
  else if (c.shape == 2) launch_ig<2, 4, 4, 2, 2, false>(a, c);
  else if (c.shape == 1) c.stages == 1 ? launch_ig128<2, 1>(a, c, out_f32) : launch_ig128<2, 2>(a, c, out_f32);
  else c.stages == 1 ? launch_ig128<1, 1>(a, c, out_f32) : launch_ig128<1, 2>(a, c, out_f32);
  return check_launch(what);
}

// geometry of the data gradient as the launch sees it: BFHIP_CONV_DGRAD_PARITY=0 keeps strided layers on the plain transposed
// gather (MODE 1) instead of the parity classes (MODE 2).  One function for the launch and for bfhip_conv2d_launch_choice
ConvGeom dgrad_geom(int N, int H, int W, int Cin, int ldx, int Cout, int ldg, int KH, int KW, int stride, int pad, int dil) {
  static const int parity = env_int("BFHIP_CONV_DGRAD_PARITY", 1);
  return conv_geom_dgrad(N, H, W, Cin, ldx, Cout, ldg, KH, KW, stride, pad, dil, parity != 0);
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_conv2d_supported(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil) {
  return geom_ok(N, H, W, Cin, KH, KW, stride, pad, dil) && geom_ok(N, H, W, Cout, KH, KW, stride, pad, dil) ? 1 : 0;
}

// rows of the BN-statistics partial buffer the forward writes: stat_partial f32[conv2d_stat_rows][2][Cout]
BFHIP_EXPORT int bfhip_conv2d_stat_rows(int N, int OH, int OW) { return ceil_div((long long)N * OH * OW, 128); }

// y[N, OH, OW, Cout] (pixel pitch ldy) = conv(x[N, H, W, Cin] (pixel pitch ldx), w[Cout][KH][KW][Cin]) (+ bias); bf16 in,
// bf16 or fp32 out.  stat_partial (optional): f32[ceil(M / 128)][2][Cout] per-row-block column sums / sums of squares of the
// un-biased fp32 accumulators (the `partial` input of bfhip_bn2d_fwd_partials).
BFHIP_EXPORT int bfhip_conv2d_fwd(const void *x, int ldx, const void *w, const float *bias, void *y, int ldy, int N, int H, int W,
                                  int Cin, int Cout, int KH, int KW, int stride, int pad, int dil, int out_f32,
                                  float *stat_partial, void *stream_) {
  BFHIP_REQUIRE(bfhip_conv2d_supported(N, H, W, Cin, Cout, KH, KW, stride, pad, dil), "conv2d_fwd: unsupported geometry");
  BFHIP_REQUIRE(x && w && y, "conv2d_fwd: null pointer");
  BFHIP_REQUIRE(dma_operand_ok(x, ldx, Cin) && ((uintptr_t)w % 16) == 0 && ldy >= Cout, kOperandMsg, "conv2d_fwd");
  const ConvGeom g = conv_geom_fwd(N, H, W, Cin, ldx, Cout, KH, KW, stride, pad, dil, ldy);
  BFHIP_REQUIRE(g.OH > 0 && g.OW > 0, "conv2d_fwd: empty output");
  BFHIP_REQUIRE((long long)N * H * W * ldx < (1LL << 31), "conv2d_fwd: tensors of 2^31 elements or more are not supported");
  ProfScope ps;
  prof_begin(takes_pointwise(g) ? BFHIP_OP_CONV2D_PW_FWD : BFHIP_OP_CONV2D_FWD, (hipStream_t)stream_, &ps);
  const int rc = launch_igemm(x, w, bias, y, stat_partial, g, out_f32, (hipStream_t)stream_, "conv2d_fwd");
  prof_end(&ps);
  return rc;
}

// Which kernel bfhip_conv2d_fwd (dir 0) / bfhip_conv2d_dgrad(_wt) (dir 1) would launch for this geometry in this process (knobs
// and CU count included): the geometry builders and choose_igemm of the launch path, no launch, no device needed.
// out_host[8] = {pointwise, shape (pointwise: BN), stages, gather mode (ConvGeom::transposed), BM, BN, tiles_m, tiles_n}
BFHIP_EXPORT int bfhip_conv2d_launch_choice(int dir, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                            int dil, int out_f32, int32_t *out_host) {
  BFHIP_REQUIRE(out_host && (dir == 0 || dir == 1), "conv2d_launch_choice: bad arguments");
  BFHIP_REQUIRE(bfhip_conv2d_supported(N, H, W, Cin, Cout, KH, KW, stride, pad, dil), "conv2d_launch_choice: unsupported geometry");
  const ConvGeom g = dir ? dgrad_geom(N, H, W, Cin, Cin, Cout, Cout, KH, KW, stride, pad, dil)
                         : conv_geom_fwd(N, H, W, Cin, Cin, Cout, KH, KW, stride, pad, dil, Cout);
  BFHIP_REQUIRE((dir ? g.H > 0 && g.W > 0 : g.OH > 0 && g.OW > 0), "conv2d_launch_choice: empty output");
  const IgemmChoice c = choose_igemm(g, out_f32, device_cus());
  const int32_t v[8] = {c.pointwise ? 1 : 0, c.pointwise ? c.BN : c.shape, c.stages, g.transposed, c.BM, c.BN, c.tiles_m, c.tiles_n};
  for (int i = 0; i < 8; ++i) out_host[i] = v[i];
  return BFHIP_OK;
}

BFHIP_EXPORT size_t bfhip_conv2d_dgrad_workspace_bytes(int Cin, int Cout, int KH, int KW) {
  return align_up((size_t)Cin * KH * KW * Cout * 2, 256);
}

// dx[N, H, W, Cin] = conv_transpose(dy[N, OH, OW, Cout], w): the forward kernel in transposed-gather mode over the
// [Cin][KH][KW][Cout] transpose of the weight (built in `workspace`).
// w: the convolution's weight (transposed into `workspace` first) or, with w == nullptr, `workspace` IS the transposed weight
static int conv2d_dgrad_impl(const void *dy, int ldg, const void *w, void *dx, int ldx, int N, int H, int W, int Cin, int Cout,
                             int KH, int KW, int stride, int pad, int dil, int out_f32, void *workspace, size_t workspace_bytes,
                             hipStream_t s, const void *addend = nullptr, int addend_stride = 1) {
  BFHIP_REQUIRE(bfhip_conv2d_supported(N, H, W, Cin, Cout, KH, KW, stride, pad, dil), "conv2d_dgrad: unsupported geometry");
  BFHIP_REQUIRE(dy && dx && workspace, "conv2d_dgrad: null pointer");
  BFHIP_REQUIRE(workspace_bytes >= bfhip_conv2d_dgrad_workspace_bytes(Cin, Cout, KH, KW), "conv2d_dgrad: workspace too small");
  BFHIP_REQUIRE(dma_operand_ok(dy, ldg, Cout) && ((uintptr_t)workspace % 16) == 0 && ldx >= Cin, kOperandMsg, "conv2d_dgrad");
  const ConvGeom g = dgrad_geom(N, H, W, Cin, ldx, Cout, ldg, KH, KW, stride, pad, dil);
  BFHIP_REQUIRE((long long)N * g.H * g.W * ldg < (1LL << 31), "conv2d_dgrad: tensors of 2^31 elements or more are not supported");
  BFHIP_REQUIRE(((uintptr_t)addend % 4) == 0 && (addend_stride == 1 || addend_stride == 2), "conv2d_dgrad: bad addend");
  ProfScope ps;
  prof_begin(takes_pointwise(g) ? BFHIP_OP_CONV2D_PW_DGRAD : BFHIP_OP_CONV2D_DGRAD, s, &ps);
  if (w)
    hipLaunchKernelGGL(conv_weight_transpose_kernel, dim3(ceil_div(Cin, 32), ceil_div(Cout, 32), KH * KW), dim3(256), 0, s,
                       (const bf16_t *)w, (bf16_t *)workspace, Cout, KH * KW, Cin);
  const int rc = launch_igemm(dy, workspace, nullptr, dx, nullptr, g, out_f32, s, "conv2d_dgrad",
                              Addend{(const bf16_t *)addend, addend ? addend_stride : 0, Cin, H, W});
  prof_end(&ps);
  return rc;
}

BFHIP_EXPORT int bfhip_conv2d_dgrad(const void *dy, int ldg, const void *w, void *dx, int ldx, int N, int H, int W, int Cin,
                                    int Cout, int KH, int KW, int stride, int pad, int dil, int out_f32, void *workspace,
                                    size_t workspace_bytes, void *stream_) {
  BFHIP_REQUIRE(w, "conv2d_dgrad: null pointer");
  return conv2d_dgrad_impl(dy, ldg, w, dx, ldx, N, H, W, Cin, Cout, KH, KW, stride, pad, dil, out_f32, workspace, workspace_bytes,
                           (hipStream_t)stream_);
}

// the same with the weight already transposed: wt bf16 [Cin][KH][KW][Cout] (bfhip_conv2d_weight_transpose_batched); read-only.
// addend (optional, bf16, dense: pixel pitch Cin): dx = data gradient + addend in the kernel's epilogue -- the other gradient path
// into the same tensor (a residual connection).  addend_stride 1: addend is [N, H, W, Cin]; 2: addend is [N, ceil(H/2), ceil(W/2), Cin],
// the gradient of a stride-2 1x1 shortcut over x, and reaches the pixels with even h and w only.  Only for calls the pointwise
// kernel serves (bfhip_conv2d_dgrad_fuses_addend)
BFHIP_EXPORT int bfhip_conv2d_dgrad_wt(const void *dy, int ldg, const void *wt, const void *addend, int addend_stride, void *dx,
                                       int ldx, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                                       int out_f32, void *stream_) {
  return conv2d_dgrad_impl(dy, ldg, nullptr, dx, ldx, N, H, W, Cin, Cout, KH, KW, stride, pad, dil, out_f32, (void *)wt,
                           bfhip_conv2d_dgrad_workspace_bytes(Cin, Cout, KH, KW), (hipStream_t)stream_, addend, addend_stride);
}

BFHIP_EXPORT int bfhip_conv2d_dgrad_fuses_addend(int KH, int KW, int stride, int pad, int out_f32) {
  return KH == 1 && KW == 1 && stride == 1 && pad == 0 && !out_f32 ? 1 : 0;
}

// src f32 [P][C] (dense) -> bf16 pairs hi / lo (v ~ hi + lo to 2^-16 relative): chan (optional) bf16 [P][3C], batch (optional)
// bf16 [3][P][C]; bit k of order_* = block k holds lo.  C % 8 == 0.
BFHIP_EXPORT int bfhip_split_bf16x3(const float *src, long long P, int C, void *chan, int order_chan, void *batch, int order_batch,
                                    void *stream_) {
  BFHIP_REQUIRE(src && (chan || batch) && P > 0 && C > 0 && C % 8 == 0, "split_bf16x3: bad arguments");
  BFHIP_REQUIRE(((uintptr_t)src % 16) == 0 && ((uintptr_t)chan % 16) == 0 && ((uintptr_t)batch % 16) == 0, "split_bf16x3: misaligned tensor");
  const long long total = P * (C / 8);
  BFHIP_REQUIRE(total < (1LL << 31) * 256, "split_bf16x3: tensor too large");
  hipLaunchKernelGGL(split_bf16x3_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream_, src, P, C,
                     (bf16_t *)chan, order_chan, (bf16_t *)batch, order_batch);
  return check_launch("split_bf16x3");
}

BFHIP_EXPORT int bfhip_conv2d_wt_segment_bytes(void) { return (int)sizeof(WtSeg); }

// segs_dev: nseg device records {u64 src, u64 dst, i32 Cout, i32 taps, i32 Cin, i32 src_f32, i64 first block}, blocks of a
// segment = ceil(Cin / 32) * ceil(Cout / 32) * taps, first blocks ascending from 0; total_blocks = their sum
BFHIP_EXPORT int bfhip_conv2d_weight_transpose_batched(const void *segs_dev, int nseg, long long total_blocks, void *stream_) {
  BFHIP_REQUIRE(segs_dev && nseg > 0 && total_blocks > 0 && total_blocks < (1LL << 31), "conv2d_weight_transpose_batched: bad table");
  hipLaunchKernelGGL(conv_weight_transpose_batched_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream_,
                     (const WtSeg *)segs_dev, nseg);
  return check_launch("conv2d_weight_transpose_batched");
}
