// conv2d_wgrad.hip -- weight gradient of the dense 2-D convolution (conv2d.hip) on the gfx950 matrix cores.
//
// dW[co][k] = sum_m dy[m][co] * A[m][k], m = (n, oh, ow), k = (kh, kw, ci), reduces over pixels: both operands are staged
// pixel-major (A gathered piece by piece, as in the forward) and read with the transposing LDS read of wgrad_tr.h, the pixel
// range is split over workgroups and the fp32 partial slabs are summed in a fixed order.
#include "wgrad_tr.h"
#include <string.h>
#include <algorithm>
#include <vector>

namespace bfhip {
namespace {

struct WgradGeom {
  ConvGeom c;      // forward geometry of the conv (gathered tensor = x)
  int Cout, ldg;   // dy channels and pixel pitch
  int splits;      // pixel range split
  long long rows_per_split;  // multiple of 64
  int tiles_co, tiles_k;
};

__global__ __launch_bounds__(256, 2) void conv_wgrad_kernel(const bf16_t *__restrict__ x, const bf16_t *__restrict__ dy,
                                                            float *__restrict__ slab, WgradGeom wg) {
  constexpr int BP = 64, T_BYTES = BP * 256;  // one tile: 64 pixels x 128 columns bf16
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  unsigned char *sG = smem, *sX = smem + 2 * T_BYTES;
  unsigned *taps = (unsigned *)(smem + 4 * T_BYTES);
  const ConvGeom &g = wg.c;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tiles = wg.tiles_co * wg.tiles_k;
  const long long lb = xcd_chunked_block(blockIdx.x, (long long)tiles * wg.splits);
  const int split = (int)(lb / tiles), tile = (int)(lb - (long long)split * tiles);
  const int tco = tile / wg.tiles_k, tk = tile - tco * wg.tiles_k;
  const int co0 = tco * 128, q0 = tk * 16;  // first dy channel, first K piece of this tile
  build_tap_table(taps, g);

  const long long p_begin = (long long)split * wg.rows_per_split;
  long long p_end = p_begin + wg.rows_per_split;
  if (p_end > g.M) p_end = g.M;
  const int nsteps = p_end > p_begin ? (int)((p_end - p_begin + BP - 1) / BP) : 0;

  // staging: one DMA instruction = 4 rows x 256 B; wave w stages rows [16w, 16w + 16): instruction i -> row 16w + 4i + (lane >> 4)
  const int lrow = lane >> 4, lpos = lane & 15;
  int pn[4], poh[4], pow_[4];  // pixel coordinates of this lane's 4 rows (advanced by 64 pixels per step)
  long long pm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long long m = p_begin + w * 16 + i * 4 + lrow;
    pm[i] = m;
    long long mm = m < g.M ? m : 0;
    int n = (int)(mm / ((long long)g.OH * g.OW));
    int rem = (int)(mm - (long long)n * g.OH * g.OW);
    pn[i] = n;
    poh[i] = rem / g.OW;
    pow_[i] = rem - poh[i] * g.OW;
  }
  __syncthreads();

  // a lane's pieces are fixed for the whole kernel: dy channel block / K piece (tap, ci) of row i
  int pdh[4], pdw[4], pcx[4];
  bool qok[4], cok[4];
  const bf16_t *gsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = w * 16 + i * 4 + lrow;
    const int c = lpos ^ tr_swz(r);
    const int co = co0 + c * 8, q = q0 + c;
    cok[i] = co < wg.Cout;
    qok[i] = q < g.nq;
    const unsigned info = qok[i] ? taps[q] : 0u;
    pdh[i] = info >> 24;
    pdw[i] = (info >> 16) & 0xff;
    pcx[i] = info & 0xffff;
    gsrc[i] = dy + ((size_t)pm[i] * wg.ldg + co);
  }
  const bf16_t *zsrc = zero_src();
  auto stage = [&](int buf) {
    unsigned char *dG = sG + buf * T_BYTES + (w * 16) * 256, *dX = sX + buf * T_BYTES + (w * 16) * 256;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool rok = pm[i] < p_end;
      glds16((rok && cok[i]) ? gsrc[i] : zsrc, dG + i * 1024);
      const int ih = poh[i] * g.stride - g.pad + pdh[i], iw = pow_[i] * g.stride - g.pad + pdw[i];
      const bool ok = rok && qok[i] && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
      const bf16_t *sx = ok ? x + ((size_t)((pn[i] * g.H + ih) * g.W + iw) * g.ldx + pcx[i]) : zsrc;
      glds16(sx, dX + i * 1024);
    }
  };
  auto advance = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pm[i] += BP;
      gsrc[i] += (size_t)BP * wg.ldg;
      pow_[i] += BP;
      while (pow_[i] >= g.OW) { pow_[i] -= g.OW; ++poh[i]; }
      while (poh[i] >= g.OH) { poh[i] -= g.OH; ++pn[i]; }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int wm = w >> 1, wn = w & 1;
  const TrAddr ad = tr_addresses(lane, wm, wn);

  if (nsteps > 0) stage(0);
  for (int t = 0; t < nsteps; ++t) {
    const int buf = t & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // raw: __syncthreads() would add its own vmcnt(0) lgkmcnt(0) (harmless here, not in the ring below)
    if (t + 1 < nsteps) { advance(); stage(buf ^ 1); }
    const unsigned char *pG = sG + buf * T_BYTES, *pX = sX + buf * T_BYTES;
    tr_compute_step(pG, pX, ad, acc);
  }

  const int Ktot = g.nq * 8;
  tr_store_slab(slab + (size_t)split * wg.Cout * Ktot, wg.Cout, Ktot, co0, q0, lane, wm, wn, acc);
}

// Round 3: the same weight gradient on wider tiles with a three-stage ring.  The 128 x 128 kernel above runs two workgroups
// per CU with ONE 32 KB stage in flight each, issued only after the previous one has landed: ~36 KB in flight per CU on
// average, 44 GB/s per CU of L2 -> LDS fill (the guide's gather-into-LDS rate with 72 KB in flight is 66-73), MFMA 30 % busy.
// Here a workgroup owns (PG * 128) dy channels x (PX * 128) K columns -- PG + PX "panels" of 64 pixels x 128 columns per
// stage, each panel laid out exactly like the tiles above, (2 PG) x (2 PX) waves of 64 x 64 -- and keeps TWO stages in
// flight behind the one being consumed (wait = vmcnt(pieces of one stage), one barrier per step): <1, 2> and <2, 1> move
// 3/4 of the operand bytes per flop of the 128 x 128 tile with 96 KB continuously in flight per CU.
// `lb`: this workgroup's index among the tiles_co * tiles_k * splits workgroups of the layer (split-major), `smem`: the dynamic LDS
template <int PG, int PX, int STAGES>
__device__ __forceinline__ void wgrad_wide_body(const bf16_t *__restrict__ x, const bf16_t *__restrict__ dy,
                                                float *__restrict__ slab, const WgradGeom &wg, const long long lb,
                                                unsigned char *smem) {
  constexpr int W = 4 * PG * PX;            // waves
  constexpr int GPW = 16 / W;               // 4-row groups of a 64-pixel stage staged by one wave
  static_assert(GPW >= 1 && GPW * W == 16, "waves must divide the 16 row groups of a stage");
  constexpr int BP = 64, PANEL = BP * 256;  // one panel: 64 pixels x 128 columns bf16
  constexpr int SB = (PG + PX) * PANEL;     // bytes of one stage
  constexpr int PER_STAGE = GPW * (PG + PX);  // DMA instructions per wave and stage
  unsigned *taps = (unsigned *)(smem + STAGES * SB);
  const ConvGeom &g = wg.c;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave index in an SGPR
  const int tiles = wg.tiles_co * wg.tiles_k;
  const int split = (int)(lb / tiles), tile = (int)(lb - (long long)split * tiles);
  const int tco = tile / wg.tiles_k, tk = tile - tco * wg.tiles_k;
  const int co0 = tco * (128 * PG), q0 = tk * (16 * PX);  // first dy channel, first K piece of this tile
  build_tap_table(taps, g);

  const long long p_begin = (long long)split * wg.rows_per_split;
  long long p_end = p_begin + wg.rows_per_split;
  if (p_end > g.M) p_end = g.M;
  const int nsteps = p_end > p_begin ? (int)((p_end - p_begin + BP - 1) / BP) : 0;

  // staging: one DMA instruction = 4 rows x 256 B of one panel; wave w stages row groups [GPW * w, GPW * (w + 1)) of EVERY panel.
  // Address generation is incremental and 32-bit (the host checks that both tensors have < 2^31 elements and OH * OW >= 64):
  // a piece's source is x + xb[row group] + xoff[slot] with xb = ((n*H + oh*stride - pad)*W + ow*stride - pad)*ldx moved by a
  // constant per step plus one correction per row / image wrap, and xoff = (dh*W + dw)*ldx + ci fixed for the whole kernel --
  // no multiply and no division inside the loop (round 2's form spent ~150 vector instructions per wave and step here, several
  // of them quarter-rate 64-bit multiplies, beside 16 MFMAs).
  const int lrow = lane >> 4, lpos = lane & 15;
  int rem[GPW], hb[GPW], wb[GPW], xb[GPW], gb[GPW];
#pragma unroll
  for (int i = 0; i < GPW; ++i) {
    const long long m = p_begin + (GPW * w + i) * 4 + lrow;
    rem[i] = (int)(p_end - m);
    const long long mm = m < g.M ? m : 0;
    const int n = (int)(mm / ((long long)g.OH * g.OW));
    const int r2 = (int)(mm - (long long)n * g.OH * g.OW);
    const int oh = r2 / g.OW, ow = r2 - oh * g.OW;
    hb[i] = oh * g.stride - g.pad;
    wb[i] = ow * g.stride - g.pad;
    xb[i] = ((n * g.H + hb[i]) * g.W + wb[i]) * g.ldx;
    gb[i] = (int)mm * wg.ldg;
  }
  const int q64 = BP / g.OW, r64 = BP - q64 * g.OW;
  const int adv_h = q64 * g.stride, adv_w = r64 * g.stride;
  const int adv_x = (adv_h * g.W + adv_w) * g.ldx;
  const int wlim = g.OW * g.stride - g.pad, hlim = g.OH * g.stride - g.pad;
  const int wrap_w = g.OW * g.stride, wrap_h = g.OH * g.stride;
  const int fix_w = (g.stride * g.W - wrap_w) * g.ldx;        // ow: OW -> 0, oh + 1
  const int fix_h = (g.H * g.W - wrap_h * g.W) * g.ldx;       // oh: OH -> 0, n + 1
  const int adv_g = BP * wg.ldg;
  __syncthreads();  // tap table ready

  // a lane's pieces are fixed for the whole kernel: dy channel block of G panel p / K piece (tap, ci) of X panel p, row group i
  int xoff[GPW][PX], xdh[GPW][PX], xdw[GPW][PX], gco[GPW][PG];
  bool qok[GPW][PX], cok[GPW][PG];
#pragma unroll
  for (int i = 0; i < GPW; ++i) {
    const int r = (GPW * w + i) * 4 + lrow;
    const int c = lpos ^ tr_swz(r);
#pragma unroll
    for (int p = 0; p < PG; ++p) {
      gco[i][p] = co0 + p * 128 + c * 8;
      cok[i][p] = gco[i][p] < wg.Cout;
    }
#pragma unroll
    for (int p = 0; p < PX; ++p) {
      const int q = q0 + p * 16 + c;
      qok[i][p] = q < g.nq;
      const unsigned info = qok[i][p] ? taps[q] : 0u;
      xdh[i][p] = (int)(info >> 24);
      xdw[i][p] = (int)((info >> 16) & 0xff);
      xoff[i][p] = (xdh[i][p] * g.W + xdw[i][p]) * g.ldx + (int)(info & 0xffff);
    }
  }
  const bf16_t *zsrc = zero_src();
  auto stage = [&](int buf) {
    unsigned char *base = smem + buf * SB;
#pragma unroll
    for (int i = 0; i < GPW; ++i) {
      const bool rok = rem[i] > 0;
      const int rowoff = ((GPW * w + i) * 4) * 256;
#pragma unroll
      for (int p = 0; p < PG; ++p)
        glds16((rok && cok[i][p]) ? dy + (unsigned)(gb[i] + gco[i][p]) : zsrc, base + p * PANEL + rowoff);
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const bool ok = rok && qok[i][p] && (unsigned)(hb[i] + xdh[i][p]) < (unsigned)g.H &&
                        (unsigned)(wb[i] + xdw[i][p]) < (unsigned)g.W;
        glds16(ok ? x + (unsigned)(xb[i] + xoff[i][p]) : zsrc, base + (PG + p) * PANEL + rowoff);
      }
    }
  };
  auto advance = [&]() {
#pragma unroll
    for (int i = 0; i < GPW; ++i) {
      rem[i] -= BP;
      gb[i] += adv_g;
      int dx = adv_x;
      wb[i] += adv_w;
      hb[i] += adv_h;
      if (wb[i] >= wlim) { wb[i] -= wrap_w; hb[i] += g.stride; dx += fix_w; }
      if (hb[i] >= hlim) { hb[i] -= wrap_h; dx += fix_h; }
      xb[i] += dx;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int wm = w / (2 * PX), wn = w % (2 * PX);
  const TrAddr ad = tr_addresses(lane, wm & 1, wn & 1);
  const int offG = (wm >> 1) * PANEL, offX = (PG + (wn >> 1)) * PANEL;

  // prologue: STAGES - 1 stages in flight
#pragma unroll
  for (int s0 = 0; s0 < STAGES - 1; ++s0)
    if (s0 < nsteps) {
      if (s0 > 0) advance();
      stage(s0);
    }
  for (int t = 0; t < nsteps; ++t) {
    const int buf = t % STAGES;
    // stage t has landed when at most the younger stages' pieces are outstanding
    if (STAGES == 3 && t + 1 < nsteps) wait_vmcnt<PER_STAGE>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();  // raw barrier: __syncthreads() drains vmcnt to 0 and with it the stage just prefetched
    if (t + STAGES - 1 < nsteps) { advance(); stage((t + STAGES - 1) % STAGES); }
    const unsigned char *pS = smem + buf * SB;
    tr_compute_step(pS + offG, pS + offX, ad, acc);
  }

  const int Ktot = g.nq * 8;
  tr_store_slab(slab + (size_t)split * wg.Cout * Ktot, wg.Cout, Ktot, co0, q0, lane, wm, wn, acc);
}

template <int PG, int PX, int STAGES>
__global__ __launch_bounds__(PG * PX * 256, 1) void conv_wgrad_wide_kernel(const bf16_t *__restrict__ x,
                                                                           const bf16_t *__restrict__ dy,
                                                                           float *__restrict__ slab, WgradGeom wg) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const long long lb = xcd_chunked_block(blockIdx.x, (long long)wg.tiles_co * wg.tiles_k * wg.splits);
  wgrad_wide_body<PG, PX, STAGES>(x, dy, slab, wg, lb, smem);
}

// ---- Grouped weight gradients: the layers of a whole backward pass in ONE launch per tile shape.  dW of a layer is a leaf of the
// backward graph, so the host (conv2d.py) only collects (x, dy, dW) during the backward and launches the group when the pass ends.
// Launched one by one, each layer is cut into exactly one residency round (256 workgroups): 6-9 steps of 64 pixels per workgroup
// on the ~50 small layers of the ResNet trunk, where the ring's prologue, the 128 KB slab store of every workgroup and the tail of
// the launch cost more than the steps (28-45 us each at 170-310 TFLOP/s), and splits x dW fp32 slab bytes whatever the layer
// (2.2 GB written per step).  In a group every workgroup runs ~`target_steps` steps of its layer (default 96): slab bytes fall
// with the split count, and there is one tail per step instead of one per layer.
// XCD placement: hardware workgroup b runs on XCD b % 8.  The host cuts the group's workgroup list (layers in descending order
// of steps per workgroup, each layer split-major) into 8 consecutive chunks of equal total STEPS; XCD c works through chunk c in
// order, so the tiles of one split (which share their x / dy rows) meet in one L2 and the 8 XCDs finish together.
struct WgradItem {
  unsigned long long x, dy, dw;          // bf16 [N,H,W,ldx], bf16 [N,OH,OW,ldg], dW (fp32 or bf16) [Cout][KH][KW][Cin]
  unsigned long long slab_off;           // byte offset of this layer's splits x [Cout][Ktot] fp32 slabs in the group's workspace
  long long M, rows_per_split, total;    // pixels, pixels per split (multiple of 64), Cout * Ktot
  int N, H, W, C, ldx, OH, OW, KH, KW, stride, pad, dil, nq;
  int Cout, ldg, splits, tiles_co, tiles_k;
  int dw_bf16, shape;                    // shape: 1 = 128 co x 256 k, 2 = 256 co x 128 k
  int first_block, n_blocks;             // in the launch of its shape (layer-local index = logical index - first_block)
  int first_rblock, n_rblocks;           // in the reduce launch (one block = 1024 elements of dW)
};
struct WgradGroupHeader {                // first 256 bytes of the table image; the items follow
  int n_items, n_shape[3], first_item[3], blocks[3], grid[3], max_nq[3], rblocks, target_steps;
  int chunk_start[3][9];                 // logical block range of XCD c in the launch of shape s: [chunk_start[s][c], chunk_start[s][c + 1])
  unsigned long long slab_bytes;
};
static_assert(sizeof(WgradGroupHeader) <= 256, "group header must fit its 256-byte slot");

template <int PG, int PX, int STAGES>
__global__ __launch_bounds__(PG * PX * 256, 1) void conv_wgrad_group_kernel(const WgradItem *__restrict__ items, int n_items,
                                                                            const int *__restrict__ chunk_start,
                                                                            unsigned char *__restrict__ slab_base) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int lbg = chunk_start[xcd] + slot;
  if (lbg >= chunk_start[xcd + 1]) return;   // whole workgroup (uniform)
  int lo = 0, hi = n_items - 1;              // last item with first_block <= lbg
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].first_block <= lbg) lo = mid;
    else hi = mid - 1;
  }
  const WgradItem &it = items[lo];
  WgradGeom wg;
  ConvGeom &g = wg.c;
  g.N = it.N; g.H = it.H; g.W = it.W; g.C = it.C; g.ldx = it.ldx; g.OH = it.OH; g.OW = it.OW;
  g.KH = it.KH; g.KW = it.KW; g.stride = it.stride; g.pad = it.pad; g.dil = it.dil; g.nq = it.nq; g.M = it.M;
  wg.Cout = it.Cout; wg.ldg = it.ldg; wg.splits = it.splits; wg.rows_per_split = it.rows_per_split;
  wg.tiles_co = it.tiles_co; wg.tiles_k = it.tiles_k;
  wgrad_wide_body<PG, PX, STAGES>((const bf16_t *)it.x, (const bf16_t *)it.dy, (float *)(slab_base + it.slab_off), wg,
                                  (long long)(lbg - it.first_block), smem);
}

__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float *__restrict__ slab, int splits, long long total,
                                                                void *__restrict__ dw, int out_bf16) {
  wgrad_reduce_body(slab, splits, total, dw, out_bf16, blockIdx.x);
}

// every layer of a group in one launch: block -> layer by its first reduce block
__global__ __launch_bounds__(256) void conv_wgrad_group_reduce_kernel(const WgradItem *__restrict__ items, int n_items,
                                                                      const unsigned char *__restrict__ slab_base) {
  const int b = blockIdx.x;
  int lo = 0, hi = n_items - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].first_rblock <= b) lo = mid;
    else hi = mid - 1;
  }
  const WgradItem &it = items[lo];
  wgrad_reduce_body((const float *)(slab_base + it.slab_off), it.splits, it.total, (void *)it.dw, it.dw_bf16, b - it.first_rblock);
}

// ------------------------------------------------------------------------------------------------ host side
// Tile shape of the weight gradient: 0 = 128 x 128 (conv_wgrad_kernel, two workgroups per CU), 1 = 128 co x 256 k and
// 2 = 256 co x 128 k (conv_wgrad_wide_kernel, three stages, one 512-thread workgroup per CU).  The wide tiles need K (resp.
// Cout) beyond one 128-column panel, a tap table that fits beside three 48 KB stages, and enough pixels for >= 6 steps.
int wgrad_shape(long long M, int Cout, int Ktot, long long ohow) {
  static const int wide = env_int("BFHIP_WGRAD_WIDE", 1);
  // ohow >= 64: the wide kernel's incremental addressing assumes at most one row wrap and one image wrap per 64-pixel step
  if (!wide || Ktot / 8 > 3584 || M < 64 * 6 || ohow < 64) return 0;
  if (Ktot > 128) return 1;
  if (Cout > 128) return 2;
  // a single 128 x 128 tile of dW over very many pixels (1x1 layers with <= 128 channels on both sides; x^T y of the decoder's
  // projections): the wide kernel with half of its tile empty still beats the two-stage 128 x 128 kernel, whose 253 workgroups of
  // 4 waves leave one wave per SIMD (BFHIP_WGRAD_WIDE_SMALL_M: fewest pixels for that, 0 = never)
  static const long long small_m = env_ll("BFHIP_WGRAD_WIDE_SMALL_M", 1024LL);
  if (small_m > 0 && M >= small_m) return 1;
  return 0;
}

// tile shape (returned), tiles and pixel split of one layer over M pixels, ohow per image (the other fields of `wg` are the caller's)
int wgrad_plan(long long M, long long ohow, int Cout, int Ktot, WgradGeom &wg) {
  const int shape = wgrad_shape(M, Cout, Ktot, ohow);
  wg.tiles_co = ceil_div(Cout, shape == 2 ? 256 : 128);
  wg.tiles_k = ceil_div(Ktot, shape == 1 ? 256 : 128);
  // 128 x 128: two workgroups per CU (66 KB of LDS each), at least 8 steps per workgroup; wide: one workgroup per CU
  // (3 x 48 KB of LDS), at least 6 steps (the ring is 3 deep; BFHIP_WGRAD_MIN_STEPS)
  static const int min_wide = env_pos_int("BFHIP_WGRAD_MIN_STEPS", 6);
  const SplitPlan p = plan_splits((M + 63) / 64, wg.tiles_co * wg.tiles_k, shape ? device_cus() : 2 * device_cus(), shape ? min_wide : 8);
  wg.splits = p.splits;
  wg.rows_per_split = p.rows_per_split;
  return shape;
}

// operand checks and forward geometry of one layer's weight gradient
int wgrad_geom(const char *what, const void *x, int ldx, const void *dy, int ldg, int N, int H, int W, int Cin, int Cout, int KH,
               int KW, int stride, int pad, int dil, ConvGeom *g) {
  BFHIP_REQUIRE(dma_operand_ok(x, ldx, Cin) && dma_operand_ok(dy, ldg, Cout), kOperandMsg, what);
  *g = conv_geom_fwd(N, H, W, Cin, ldx, Cout, KH, KW, stride, pad, dil, 0);
  BFHIP_REQUIRE((long long)N * H * W * ldx < (1LL << 31) && g->M * ldg < (1LL << 31),
                "%s: tensors of 2^31 elements or more are not supported", what);
  return BFHIP_OK;
}

constexpr int kWideLdsLimit = 160 * 1024;
inline size_t wide_lds_bytes(int nq) { return (size_t)3 * 3 * 64 * 256 + (size_t)nq * 4; }  // three stages of three panels + tap table

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT size_t bfhip_conv2d_wgrad_workspace_bytes(int N, int OH, int OW, int Cin, int Cout, int KH, int KW) {
  WgradGeom wg;
  wgrad_plan((long long)N * OH * OW, (long long)OH * OW, Cout, KH * KW * Cin, wg);
  return align_up((size_t)wg.splits * Cout * KH * KW * Cin * sizeof(float), 256);
}

// The plan bfhip_conv2d_wgrad would launch for this geometry in this process (wgrad_plan of the launch path; host only):
// out_host[4] = {tile shape (wgrad_shape), tiles_co, tiles_k, splits}
BFHIP_EXPORT int bfhip_conv2d_wgrad_choice(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil,
                                           int32_t *out_host) {
  BFHIP_REQUIRE(out_host, "conv2d_wgrad_choice: bad arguments");
  BFHIP_REQUIRE(bfhip_conv2d_supported(N, H, W, Cin, Cout, KH, KW, stride, pad, dil), "conv2d_wgrad_choice: unsupported geometry");
  const ConvGeom g = conv_geom_fwd(N, H, W, Cin, Cin, Cout, KH, KW, stride, pad, dil, 0);
  BFHIP_REQUIRE(g.OH > 0 && g.OW > 0, "conv2d_wgrad_choice: empty output");
  WgradGeom wg;
  out_host[0] = wgrad_plan(g.M, (long long)g.OH * g.OW, Cout, KH * KW * Cin, wg);
  out_host[1] = wg.tiles_co; out_host[2] = wg.tiles_k; out_host[3] = wg.splits;
  return BFHIP_OK;
}

// dw[Cout][KH][KW][Cin] (fp32 or bf16) = sum over pixels of dy x gathered x
BFHIP_EXPORT int bfhip_conv2d_wgrad(const void *x, int ldx, const void *dy, int ldg, void *dw, int N, int H, int W, int Cin,
                                    int Cout, int KH, int KW, int stride, int pad, int dil, int dw_bf16, void *workspace,
                                    size_t workspace_bytes, void *stream_) {
  hipStream_t s = (hipStream_t)stream_;
  BFHIP_REQUIRE(bfhip_conv2d_supported(N, H, W, Cin, Cout, KH, KW, stride, pad, dil), "conv2d_wgrad: unsupported geometry");
  BFHIP_REQUIRE(x && dy && dw && workspace, "conv2d_wgrad: null pointer");
  WgradGeom wg;
  ConvGeom &g = wg.c;
  if (const int rc = wgrad_geom("conv2d_wgrad", x, ldx, dy, ldg, N, H, W, Cin, Cout, KH, KW, stride, pad, dil, &g)) return rc;
  wg.Cout = Cout; wg.ldg = ldg;
  const int shape = wgrad_plan(g.M, (long long)g.OH * g.OW, Cout, KH * KW * Cin, wg);
  BFHIP_REQUIRE(workspace_bytes >= bfhip_conv2d_wgrad_workspace_bytes(N, g.OH, g.OW, Cin, Cout, KH, KW), "conv2d_wgrad: workspace too small");
  ProfScope ps;
  prof_begin(BFHIP_OP_CONV2D_WGRAD, s, &ps);
  const dim3 grid((unsigned)((long long)wg.tiles_co * wg.tiles_k * wg.splits));
  const bf16_t *xb = (const bf16_t *)x, *gb = (const bf16_t *)dy;
  if (shape == 0)
    launch_big_lds<conv_wgrad_kernel>(kWideLdsLimit / 2, grid, dim3(256), (size_t)4 * 64 * 256 + (size_t)g.nq * 4, s, xb, gb, (float *)workspace, wg);
  else if (shape == 1)
    launch_big_lds<conv_wgrad_wide_kernel<1, 2, 3>>(kWideLdsLimit, grid, dim3(512), wide_lds_bytes(g.nq), s, xb, gb, (float *)workspace, wg);
  else
    launch_big_lds<conv_wgrad_wide_kernel<2, 1, 3>>(kWideLdsLimit, grid, dim3(512), wide_lds_bytes(g.nq), s, xb, gb, (float *)workspace, wg);
  const long long total = (long long)Cout * KH * KW * Cin;
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(ceil_div(total, 1024)), dim3(256), 0, s, (const float *)workspace, wg.splits,
                     total, dw, dw_bf16);
  prof_end(&ps);
  return check_launch("conv2d_wgrad");
}

// ---------------------------------------------------------------------------------- grouped weight gradients (host side)
// One record per layer, filled by the caller in host memory (include/bevfusion_hip.h: bfhip_wgrad_layer).
struct WgradLayerDesc {
  const void *x, *dy;
  void *dw;
  int ldx, ldg, N, H, W, Cin, Cout, KH, KW, stride, pad, dil, dw_bf16, reserved;
};
static_assert(sizeof(WgradLayerDesc) == 80, "bfhip_wgrad_layer layout");

BFHIP_EXPORT size_t bfhip_conv2d_wgrad_group_table_bytes(int n_layers) {
  return n_layers > 0 ? 256 + (size_t)n_layers * sizeof(WgradItem) : 0;
}

// 1 when the layer can join a group: a geometry the wide weight-gradient kernels take (everything else keeps bfhip_conv2d_wgrad)
BFHIP_EXPORT int bfhip_conv2d_wgrad_groupable(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int dil) {
  if (!bfhip_conv2d_supported(N, H, W, Cin, Cout, KH, KW, stride, pad, dil)) return 0;
  const int OH = conv_out_dim(H, KH, stride, pad, dil), OW = conv_out_dim(W, KW, stride, pad, dil);
  return wgrad_shape((long long)N * OH * OW, Cout, KH * KW * Cin, (long long)OH * OW) != 0;
}

// Plans the group and writes the image of its device table (header + one item per layer) into table_host; the caller copies
// the image to the device (stream-ordered, before the launch) and provides *slab_bytes of workspace.  target_steps: 64-pixel
// steps per workgroup to aim for (<= 0: BFHIP_WGRAD_GROUP_STEPS or 96: the 77 layers of the full step at 32 / 64 / 96 / 128 / 192 / 256 steps take 3.29 / 2.95 /
// 2.80 / 2.80 / 2.83 / 2.84 ms with 1.9 / 1.0 / 0.73 / 0.58 / 0.44 / 0.36 GB of slabs; inside the full step, ten alternating pairs: 96
// steps 25.9 ms, 192 steps 26.3 ms (median) -- the last residency round of 192-step workgroups is a 260 us tail).
BFHIP_EXPORT int bfhip_conv2d_wgrad_group_plan(const void *layers_, int n, int target_steps, void *table_host, size_t table_bytes,
                                               size_t *slab_bytes) {
  const WgradLayerDesc *L = (const WgradLayerDesc *)layers_;
  BFHIP_REQUIRE(L && n > 0 && table_host && slab_bytes, "conv2d_wgrad_group_plan: bad arguments");
  BFHIP_REQUIRE(table_bytes >= bfhip_conv2d_wgrad_group_table_bytes(n), "conv2d_wgrad_group_plan: table too small");
  if (target_steps <= 0) {
    static const int env = env_pos_int("BFHIP_WGRAD_GROUP_STEPS", 96);
    target_steps = env;
  }
  WgradGroupHeader hd;
  memset(&hd, 0, sizeof hd);
  hd.n_items = n;
  hd.target_steps = target_steps;
  std::vector<WgradItem> items((size_t)n);
  std::vector<long long> per((size_t)n);
  long long shape_steps[3] = {0, 0, 0};
  int shape_target[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const WgradLayerDesc &d = L[i];
    BFHIP_REQUIRE(d.x && d.dy && d.dw, "conv2d_wgrad_group_plan: null pointer in a layer");
    BFHIP_REQUIRE(bfhip_conv2d_wgrad_groupable(d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, d.pad, d.dil),
                  "conv2d_wgrad_group_plan: a layer is not groupable (ask bfhip_conv2d_wgrad_groupable first)");
    BFHIP_REQUIRE(((uintptr_t)d.dw % 16) == 0, kOperandMsg, "conv2d_wgrad_group_plan");
    WgradGeom wg;
    ConvGeom &g = wg.c;
    if (const int rc = wgrad_geom("conv2d_wgrad_group_plan", d.x, d.ldx, d.dy, d.ldg, d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW,
                                  d.stride, d.pad, d.dil, &g))
      return rc;
    WgradItem &it = items[i];
    memset(&it, 0, sizeof it);
    it.x = (unsigned long long)(uintptr_t)d.x; it.dy = (unsigned long long)(uintptr_t)d.dy; it.dw = (unsigned long long)(uintptr_t)d.dw;
    it.N = g.N; it.H = g.H; it.W = g.W; it.C = g.C; it.ldx = g.ldx; it.OH = g.OH; it.OW = g.OW;
    it.KH = g.KH; it.KW = g.KW; it.stride = g.stride; it.pad = g.pad; it.dil = g.dil; it.nq = g.nq; it.M = g.M;
    it.Cout = d.Cout; it.ldg = d.ldg; it.dw_bf16 = d.dw_bf16;
    const int Ktot = d.KH * d.KW * d.Cin;
    it.shape = wgrad_plan(g.M, (long long)g.OH * g.OW, d.Cout, Ktot, wg);  // shape and tiles; the group splits by its own rule below
    it.tiles_co = wg.tiles_co;
    it.tiles_k = wg.tiles_k;
    it.total = (long long)d.Cout * Ktot;
    it.n_rblocks = (int)ceil_div(it.total, 1024);
    shape_steps[it.shape] += (long long)it.tiles_co * it.tiles_k * ((it.M + 63) / 64);
  }
  // steps per workgroup: the target, lowered for a launch that would otherwise have fewer than ~4 residency rounds of workgroups
  // (the 9 layers with K <= 128 of the ResNet trunk at 96 steps: 285 workgroups on 256 CUs = two rounds, the second one empty)
  for (int sh = 1; sh <= 2; ++sh) {
    long long t = shape_steps[sh] / 1024;
    shape_target[sh] = (int)std::min<long long>(target_steps, std::max<long long>(8, t));
  }
  for (int i = 0; i < n; ++i) {
    WgradItem &it = items[i];
    const int tgt = shape_target[it.shape];
    const long long steps = (it.M + 63) / 64;
    long long want = (steps + tgt / 2) / tgt;
    if (want > steps / 6) want = steps / 6;  // the ring is three deep: at least 6 steps per workgroup
    if (want < 1) want = 1;
    per[i] = (steps + want - 1) / want;
    it.splits = (int)((steps + per[i] - 1) / per[i]);
    it.rows_per_split = per[i] * 64;
    it.n_blocks = it.tiles_co * it.tiles_k * it.splits;
  }
  // table order: shape 1 then shape 2, inside a shape by descending steps per workgroup (ties: caller's order)
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    if (items[a].shape != items[b].shape) return items[a].shape < items[b].shape;
    return per[a] > per[b];
  });
  WgradItem *out = (WgradItem *)((unsigned char *)table_host + 256);
  size_t slab = 0;
  long long rb = 0;
  for (int sh = 1; sh <= 2; ++sh) hd.first_item[sh] = -1;
  for (int k = 0; k < n; ++k) {
    WgradItem it = items[order[k]];
    const int sh = it.shape;
    if (hd.first_item[sh] < 0) hd.first_item[sh] = k;
    ++hd.n_shape[sh];
    it.first_block = hd.blocks[sh];
    BFHIP_REQUIRE((long long)hd.blocks[sh] + it.n_blocks < (1LL << 30), "conv2d_wgrad_group_plan: too many workgroups");
    hd.blocks[sh] += it.n_blocks;
    if (it.nq > hd.max_nq[sh]) hd.max_nq[sh] = it.nq;
    it.slab_off = slab;
    slab += align_up((size_t)it.splits * it.total * sizeof(float), 256);
    it.first_rblock = (int)rb;
    rb += it.n_rblocks;
    BFHIP_REQUIRE(rb < (1LL << 30), "conv2d_wgrad_group_plan: too many reduce blocks");
    out[k] = it;
  }
  hd.rblocks = (int)rb;
  hd.slab_bytes = slab;
  // XCD chunks of equal total steps (a workgroup's cost = its step count; all workgroups of one launch have the same tile shape)
  for (int sh = 1; sh <= 2; ++sh) {
    if (!hd.n_shape[sh]) continue;
    const WgradItem *its = out + hd.first_item[sh];
    long long total_steps = 0;
    for (int k = 0; k < hd.n_shape[sh]; ++k) total_steps += (long long)its[k].n_blocks * (its[k].rows_per_split / 64);
    int c = 1, longest = 0;
    long long acc = 0;
    hd.chunk_start[sh][0] = 0;
    for (int k = 0; k < hd.n_shape[sh]; ++k) {
      const long long w = its[k].rows_per_split / 64;
      for (int b = 0; b < its[k].n_blocks; ++b) {
        // block (first_block + b) opens chunk c when the steps before it reach c/8 of the total
        while (c < 8 && acc * 8 >= total_steps * c) hd.chunk_start[sh][c++] = its[k].first_block + b;
        acc += w;
      }
    }
    while (c <= 8) hd.chunk_start[sh][c++] = hd.blocks[sh];
    for (int x = 0; x < 8; ++x) longest = std::max(longest, hd.chunk_start[sh][x + 1] - hd.chunk_start[sh][x]);
    hd.grid[sh] = 8 * longest;
  }
  memcpy(table_host, &hd, sizeof hd);
  *slab_bytes = slab;
  return 0;
}

// table_host: the image bfhip_conv2d_wgrad_group_plan wrote (its header is read here), table_dev: its device copy
BFHIP_EXPORT int bfhip_conv2d_wgrad_group_launch(const void *table_host, const void *table_dev, void *slab, size_t slab_bytes,
                                                 void *stream_) {
  hipStream_t s = (hipStream_t)stream_;
  BFHIP_REQUIRE(table_host && table_dev && slab, "conv2d_wgrad_group_launch: null pointer");
  WgradGroupHeader hd;
  memcpy(&hd, table_host, sizeof hd);
  BFHIP_REQUIRE(hd.n_items > 0 && hd.n_items == hd.n_shape[1] + hd.n_shape[2], "conv2d_wgrad_group_launch: not a planned table");
  BFHIP_REQUIRE(slab_bytes >= hd.slab_bytes && ((uintptr_t)slab % 256) == 0, "conv2d_wgrad_group_launch: workspace too small or misaligned");
  const WgradItem *items = (const WgradItem *)((const unsigned char *)table_dev + 256);
  const int *chunks = (const int *)((const unsigned char *)table_dev + offsetof(WgradGroupHeader, chunk_start));
  ProfScope ps;
  prof_begin(BFHIP_OP_CONV2D_WGRAD, s, &ps);
  for (int sh = 1; sh <= 2; ++sh) {
    if (!hd.n_shape[sh]) continue;
    const size_t lds = wide_lds_bytes(hd.max_nq[sh]);
    if (sh == 1)
      launch_big_lds<conv_wgrad_group_kernel<1, 2, 3>>(kWideLdsLimit, dim3((unsigned)hd.grid[sh]), dim3(512), lds, s, items + hd.first_item[sh],
                                                       hd.n_shape[sh], chunks + sh * 9, (unsigned char *)slab);
    else
      launch_big_lds<conv_wgrad_group_kernel<2, 1, 3>>(kWideLdsLimit, dim3((unsigned)hd.grid[sh]), dim3(512), lds, s, items + hd.first_item[sh],
                                                       hd.n_shape[sh], chunks + sh * 9, (unsigned char *)slab);
  }
  hipLaunchKernelGGL(conv_wgrad_group_reduce_kernel, dim3((unsigned)hd.rblocks), dim3(256), 0, s, items, hd.n_items,
                     (const unsigned char *)slab);
  prof_end(&ps);
  return check_launch("conv2d_wgrad_group");
}
