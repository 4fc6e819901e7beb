// swin_attn.hip -- shifted-window multi-head self-attention of the Swin image backbone (gfx950), forward and backward.
// 7 x 7 windows of 49 tokens, head dim 32 (every published Swin size).  The cyclic shift, the window partition, the
// relative-position bias, the shifted-window mask and the softmax are all inside the kernel: a wave works on one
// (window, head) and reads the q, k, v rows of its 49 tokens straight from the [B, Hp, Wp, 3C] output of the qkv Linear
// (channel = which * C + head * 32 + d) at the positions the roll + partition would have moved them from; no rolled or
// partitioned copy of the activations exists.
//
// Orientation.  v_mfma_f32_16x16x32_bf16 has K = 32 = the head dim, and both its operands take 8 contiguous bf16 of one
// row per lane (A[row l&15][k = 8(l>>4)+j], B[k = 8(l>>4)+j][col l&15]), so q and k fragments are 16-byte global loads.
// The forward computes S^T = K Q^T: the accumulator then holds, per lane, one QUERY (column l&15) and four KEYS
// (rows 4(l>>4)+i) of each 16 x 16 tile -- the softmax of a query is a reduction inside the lane plus two xor shuffles,
// and P^T is already the B operand of O^T = V^T P^T (the sum over keys runs over the accumulator's row index; the k order
// inside an MFMA step is the permutation {tile 2s rows 4g+i, tile 2s+1 rows 4g+i}, applied to the A operand as well).
// The A operands of the second products (V^T; K^T, Q^T, dO^T in the backward) come from a wave-private transposed LDS
// image [32 d][64 tokens].  The backward recomputes P from lse in BOTH orientations (K = 32: one MFMA per tile), so that
// dQ (sum over keys) and dK, dV (sums over queries) each get the orientation whose row index is their summation index.
// Outputs are O^T / dQ^T / dK^T / dV^T tiles: a lane owns 4 consecutive channels of one token = one 8-byte store.
//
// The bias gradient is accumulated in registers over all windows a wave walks, the four waves of a workgroup are added in
// wave order through LDS, and every workgroup writes its own [49, 49] slab: dbias_partial[gridDim.x][heads][49][49].  The
// caller sums the slabs in a fixed order.  No atomics on floating-point data anywhere.
#include "common.h"

namespace bfhip {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWin = 7;            // window side
constexpr int kTok = 49;           // tokens of a window
constexpr int kHd = 32;            // head dim
constexpr int kLdT = 68;           // row pitch (bf16) of a transposed [32][64] LDS image: 136 B, 16 rows hit distinct banks
constexpr int kWaves = 4;          // waves (= windows in flight) per workgroup
constexpr int kMaxBlocks = 512;    // workgroups of a launch (2 per CU); more windows than that are walked in a loop
constexpr int kBias = kTok * kTok;
constexpr int kWaveLds = 3 * kHd * kLdT * 2 + 2 * 64 * 4;  // backward: Q^T, K^T, dO^T images + D and lse of the 64 rows

struct Geo {
  int B, Hp, Wp, heads, C, shift, nwh, nww, nwin;
  long long pitch;  // elements between consecutive tokens of qkv
  float scale;
};

__device__ __forceinline__ unsigned pack2(float lo, float hi) { return bf16_rne(lo) | (bf16_rne(hi) << 16); }
__device__ __forceinline__ uint4 ld16(const bf16_t *p) { return *(const uint4 *)p; }
__device__ __forceinline__ uint4 zero16() { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ unsigned elem(const uint4 &v, int j) {  // bf16 element j of 8 (j a compile-time constant)
  const unsigned w = j < 2 ? v.x : j < 4 ? v.y : j < 6 ? v.z : v.w;
  return (j & 1) ? (w >> 16) : (w & 0xffffu);
}
__device__ __forceinline__ f32x4 mfma(const uint4 &a, const uint4 &b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 zero4f() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }

// window-local token t (0..48) of window (b, wr, wc): row index into [B*Hp*Wp] of the token the roll(-shift) + partition
// puts there, and its mask region (3 * region_h + region_w; regions of the shifted coordinate: [0, L-7), [L-7, L-3), [L-3, L))
__device__ __forceinline__ int region1(int u, int L) { return u < L - kWin ? 0 : (u < L - 3 ? 1 : 2); }
__device__ __forceinline__ void tok_info(const Geo &g, int b, int wr, int wc, int t, int &tok, int &reg) {
  const int r = t / kWin, c = t - r * kWin;
  const int uh = wr * kWin + r, uw = wc * kWin + c;
  reg = region1(uh, g.Hp) * 3 + region1(uw, g.Wp);
  int h = uh + g.shift, w = uw + g.shift;
  if (h >= g.Hp) h -= g.Hp;
  if (w >= g.Wp) w -= g.Wp;
  tok = (b * g.Hp + h) * g.Wp + w;
}

// transposed image: X[d][t] = row t, channel d; this lane holds channels 8 lg .. 8 lg + 7 of row t
__device__ __forceinline__ void put_transposed(bf16_t *X, const uint4 &v, int lg, int t) {
#pragma unroll
  for (int j = 0; j < 8; ++j) X[(lg * 8 + j) * kLdT + t] = (bf16_t)elem(v, j);
}
// A fragment of k-step s of the product that sums over tokens: rows d = dt*16 + ln, k elements = tokens
// {32 s + 4 lg + (0..3), 32 s + 16 + 4 lg + (0..3)} -- the order in which two accumulator tiles pack into a B fragment
__device__ __forceinline__ uint4 get_transposed(const bf16_t *X, int dt, int s, int ln, int lg) {
  const bf16_t *p = X + (dt * 16 + ln) * kLdT + 32 * s + 4 * lg;
  const uint2 lo = *(const uint2 *)p, hi = *(const uint2 *)(p + 16);
  return make_uint4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ uint4 pack_tiles(const f32x4 &a, const f32x4 &b) {
  return make_uint4(pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(b[0], b[1]), pack2(b[2], b[3]));
}
__device__ __forceinline__ void st4(bf16_t *p, const f32x4 &v) { *(uint2 *)p = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3])); }

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void swin_attn_fwd_kernel(const bf16_t *__restrict__ qkv, const float *__restrict__ bias, Geo g,
                                                            bf16_t *__restrict__ out, float *__restrict__ lse) {
  __shared__ __attribute__((aligned(16))) bf16_t vt_all[kWaves][kHd * kLdT];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, ln = lane & 15, lg = lane >> 4;
  const int head = blockIdx.y;
  bf16_t *Vt = vt_all[wave];
  const float *bh = bias + (size_t)head * kBias;
  for (int win = blockIdx.x * kWaves + wave; win < g.nwin; win += gridDim.x * kWaves) {
    const int wc = win % g.nww, wr = (win / g.nww) % g.nwh, b = win / (g.nww * g.nwh);
    int tok[4], reg[4];
    uint4 qf[4], kf[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int t = mt * 16 + ln;
      const bool ok = t < kTok;
      tok_info(g, b, wr, wc, ok ? t : kTok - 1, tok[mt], reg[mt]);
      const bf16_t *p = qkv + (size_t)tok[mt] * g.pitch + head * kHd + lg * 8;
      qf[mt] = ok ? ld16(p) : zero16();
      kf[mt] = ok ? ld16(p + g.C) : zero16();
      put_transposed(Vt, ok ? ld16(p + 2 * g.C) : zero16(), lg, t);
    }
    wave_lds_sync();
    uint4 va[2][2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int s = 0; s < 2; ++s) va[dt][s] = get_transposed(Vt, dt, s, ln, lg);
    int rk[4][4];  // regions of the keys kt*16 + 4 lg + i
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ki = kt * 16 + lg * 4 + i;
        int tk;
        tok_info(g, b, wr, wc, ki < kTok ? ki : kTok - 1, tk, rk[kt][i]);
      }
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const int qi = qt * 16 + ln;
      const bool qok = qi < kTok;
      f32x4 s[4];
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        s[kt] = mfma(kf[kt], qf[qt], zero4f());  // S^T[key kt*16 + 4 lg + i][query qt*16 + ln]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ki = kt * 16 + lg * 4 + i;
          float v = -INFINITY;
          if (ki < kTok) {
            v = s[kt][i] * g.scale + (qok ? bh[qi * kTok + ki] : 0.f);
            if (g.shift > 0 && rk[kt][i] != reg[qt]) v += -100.0f;
          }
          s[kt][i] = v;
          mx = fmaxf(mx, v);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = __expf(s[kt][i] - mx);  // keys 49..63: exp(-inf) = 0
          s[kt][i] = p;
          sum += p;
        }
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
      const float inv = 1.0f / sum;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[kt][i] *= inv;
      const uint4 pb0 = pack_tiles(s[0], s[1]), pb1 = pack_tiles(s[2], s[3]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        f32x4 o = mfma(va[dt][0], pb0, zero4f());  // O^T[d = dt*16 + 4 lg + i][query qt*16 + ln]
        o = mfma(va[dt][1], pb1, o);
        if (qok) st4(out + (size_t)tok[qt] * g.C + head * kHd + dt * 16 + lg * 4, o);
      }
      if (qok && lg == 0) lse[(size_t)tok[qt] * g.heads + head] = mx + __logf(sum);
    }
    __builtin_amdgcn_wave_barrier();  // the next window's V^T overwrites this one's
  }
}

// ---------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(256) void swin_attn_bwd_kernel(const bf16_t *__restrict__ qkv, const float *__restrict__ bias,
                                                            const bf16_t *__restrict__ out, const bf16_t *__restrict__ dout,
                                                            const float *__restrict__ lse, Geo g, bf16_t *__restrict__ dqkv,
                                                            float *__restrict__ dbias_partial) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kWaves * kWaveLds];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, ln = lane & 15, lg = lane >> 4;
  const int head = blockIdx.y;
  bf16_t *Qt = (bf16_t *)(smem + wave * kWaveLds), *Kt = Qt + kHd * kLdT, *Gt = Kt + kHd * kLdT;
  float *Dl = (float *)(Gt + kHd * kLdT), *Ll = Dl + 64;
  const float *bh = bias + (size_t)head * kBias;
  const size_t C3 = (size_t)3 * g.C;
  f32x4 dbacc[4][4];  // [key tile][query tile]: rows = keys 4 lg + i, column = query ln
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) dbacc[a][c] = zero4f();

  for (int win = blockIdx.x * kWaves + wave; win < g.nwin; win += gridDim.x * kWaves) {
    const int wc = win % g.nww, wr = (win / g.nww) % g.nwh, b = win / (g.nww * g.nwh);
    int tok[4], reg[4];
    uint4 qf[4], kf[4], vf[4], gf[4];
    float Dq[4], lq[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int t = mt * 16 + ln;
      const bool ok = t < kTok;
      tok_info(g, b, wr, wc, ok ? t : kTok - 1, tok[mt], reg[mt]);
      const bf16_t *p = qkv + (size_t)tok[mt] * g.pitch + head * kHd + lg * 8;
      const size_t orow = (size_t)tok[mt] * g.C + head * kHd + lg * 8;
      qf[mt] = ok ? ld16(p) : zero16();
      kf[mt] = ok ? ld16(p + g.C) : zero16();
      vf[mt] = ok ? ld16(p + 2 * g.C) : zero16();
      gf[mt] = ok ? ld16(dout + orow) : zero16();
      const uint4 of = ok ? ld16(out + orow) : zero16();
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d += bf16_to_f32(elem(gf[mt], j)) * bf16_to_f32(elem(of, j));
      d += __shfl_xor(d, 16);
      d += __shfl_xor(d, 32);
      Dq[mt] = d;  // rowsum(dO o O) of token t
      lq[mt] = ok ? lse[(size_t)tok[mt] * g.heads + head] : 0.f;
      if (lg == 0) { Dl[t] = d; Ll[t] = lq[mt]; }
      put_transposed(Qt, qf[mt], lg, t);
      put_transposed(Kt, kf[mt], lg, t);
      put_transposed(Gt, gf[mt], lg, t);
    }
    wave_lds_sync();
    int rk[4][4];  // regions of the window-local tokens T*16 + 4 lg + i (the accumulator rows of tile T)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ki = kt * 16 + lg * 4 + i;
        int tk;
        tok_info(g, b, wr, wc, ki < kTok ? ki : kTok - 1, tk, rk[kt][i]);
      }
    // ---- orientation 1: rows = keys, column = query (ln): dbias, dQ
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const int qi = qt * 16 + ln;
      const bool qok = qi < kTok;
      f32x4 ds[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const f32x4 st = mfma(kf[kt], qf[qt], zero4f());   // S^T
        const f32x4 dpt = mfma(vf[kt], gf[qt], zero4f());  // dP^T = V dO^T
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ki = kt * 16 + lg * 4 + i;
          float d = 0.f;
          if (qok && ki < kTok) {
            float v = st[i] * g.scale + bh[qi * kTok + ki];
            if (g.shift > 0 && rk[kt][i] != reg[qt]) v += -100.0f;
            d = __expf(v - lq[qt]) * (dpt[i] - Dq[qt]);
          }
          dbacc[kt][qt][i] += d;
          ds[kt][i] = d * g.scale;
        }
      }
      const uint4 b0 = pack_tiles(ds[0], ds[1]), b1 = pack_tiles(ds[2], ds[3]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        f32x4 dq = mfma(get_transposed(Kt, dt, 0, ln, lg), b0, zero4f());  // dQ^T[d][query] = sum_key K^T[d][key] dS^T[key][query]
        dq = mfma(get_transposed(Kt, dt, 1, ln, lg), b1, dq);
        if (qok) st4(dqkv + (size_t)tok[qt] * C3 + head * kHd + dt * 16 + lg * 4, dq);
      }
    }
    // ---- orientation 2: rows = queries, column = key (ln): dK, dV
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int ki = kt * 16 + ln;
      const bool kok = ki < kTok;
      f32x4 pv[4], ds[4];
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) {
        const f32x4 s = mfma(qf[qt], kf[kt], zero4f());   // S
        const f32x4 dp = mfma(gf[qt], vf[kt], zero4f());  // dP = dO V^T
        const float4 Lr = *(const float4 *)(Ll + qt * 16 + lg * 4), Dr = *(const float4 *)(Dl + qt * 16 + lg * 4);
        const float Lrow[4] = {Lr.x, Lr.y, Lr.z, Lr.w}, Drow[4] = {Dr.x, Dr.y, Dr.z, Dr.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int qi = qt * 16 + lg * 4 + i;
          float p = 0.f;
          if (kok && qi < kTok) {
            float v = s[i] * g.scale + bh[qi * kTok + ki];
            if (g.shift > 0 && rk[qt][i] != reg[kt]) v += -100.0f;
            p = __expf(v - Lrow[i]);
          }
          pv[qt][i] = p;
          ds[qt][i] = p * (dp[i] - Drow[i]) * g.scale;
        }
      }
      const uint4 p0 = pack_tiles(pv[0], pv[1]), p1 = pack_tiles(pv[2], pv[3]);
      const uint4 d0 = pack_tiles(ds[0], ds[1]), d1 = pack_tiles(ds[2], ds[3]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        f32x4 dk = mfma(get_transposed(Qt, dt, 0, ln, lg), d0, zero4f());  // dK^T[d][key] = sum_q Q^T[d][q] dS[q][key]
        dk = mfma(get_transposed(Qt, dt, 1, ln, lg), d1, dk);
        f32x4 dv = mfma(get_transposed(Gt, dt, 0, ln, lg), p0, zero4f());  // dV^T[d][key] = sum_q dO^T[d][q] P[q][key]
        dv = mfma(get_transposed(Gt, dt, 1, ln, lg), p1, dv);
        if (kok) {
          bf16_t *dst = dqkv + (size_t)tok[kt] * C3 + g.C + head * kHd + dt * 16 + lg * 4;
          st4(dst, dk);
          st4(dst + g.C, dv);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next window's images overwrite this one's
  }
  // bias gradient of this workgroup: the four waves add in turn (fixed order), then one slab store
  __syncthreads();
  float *red = (float *)smem;
  for (int i = threadIdx.x; i < kBias; i += 256) red[i] = 0.f;
  __syncthreads();
  for (int w = 0; w < kWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int qt = 0; qt < 4; ++qt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int qi = qt * 16 + ln, ki = kt * 16 + lg * 4 + i;
            if (qi < kTok && ki < kTok) red[qi * kTok + ki] += dbacc[kt][qt][i];
          }
    }
    __syncthreads();
  }
  float *dst = dbias_partial + ((size_t)blockIdx.x * g.heads + head) * kBias;
  for (int i = threadIdx.x; i < kBias; i += 256) dst[i] = red[i];
}

inline bool shape_ok(int B, int Hp, int Wp, int heads, int window, int head_dim, int shift) {
  if (window != kWin || head_dim != kHd || (shift != 0 && shift != 3)) return false;
  if (B <= 0 || Hp <= 0 || Wp <= 0 || heads <= 0 || heads > 65535 || Hp % kWin || Wp % kWin) return false;
  return (long long)B * Hp * Wp < (1ll << 31) / 4;  // token and window indices are 32-bit
}

inline int grid_x(int B, int Hp, int Wp, int heads) {
  const long long nwin = (long long)B * (Hp / kWin) * (Wp / kWin);
  const long long cap = kMaxBlocks / heads > 0 ? kMaxBlocks / heads : 1;
  const long long want = (nwin + kWaves - 1) / kWaves;
  return (int)(want < cap ? want : cap);
}

inline Geo make_geo(int B, int Hp, int Wp, int heads, int shift, long long pitch, float scale) {
  Geo g;
  g.B = B; g.Hp = Hp; g.Wp = Wp; g.heads = heads; g.C = heads * kHd; g.shift = shift;
  g.nwh = Hp / kWin; g.nww = Wp / kWin; g.nwin = B * g.nwh * g.nww;
  g.pitch = pitch; g.scale = scale;
  return g;
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_swin_attn_supported(int B, int Hp, int Wp, int heads, int window, int head_dim, int shift) {
  return shape_ok(B, Hp, Wp, heads, window, head_dim, shift) ? 1 : 0;
}

BFHIP_EXPORT int bfhip_swin_attn_parts(int B, int Hp, int Wp, int heads) {
  return shape_ok(B, Hp, Wp, heads, kWin, kHd, 0) ? grid_x(B, Hp, Wp, heads) : 0;
}

BFHIP_EXPORT int bfhip_swin_attn_fwd(const void *qkv, long long qkv_pitch, const float *bias, int B, int Hp, int Wp, int heads,
                                     int shift, float scale, void *out, float *lse, void *stream) {
  BFHIP_REQUIRE(shape_ok(B, Hp, Wp, heads, kWin, kHd, shift), "swin_attn_fwd: unsupported B=%d Hp=%d Wp=%d heads=%d shift=%d", B, Hp, Wp,
                heads, shift);
  BFHIP_REQUIRE(qkv && bias && out && lse, "swin_attn_fwd: null pointer");
  BFHIP_REQUIRE(qkv_pitch >= 3ll * heads * kHd && qkv_pitch % 8 == 0 && ((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 8) == 0,
                "swin_attn_fwd: qkv must be 16-byte aligned with a row pitch >= 3C that is a multiple of 8");
  const Geo g = make_geo(B, Hp, Wp, heads, shift, qkv_pitch, scale);
  hipLaunchKernelGGL(swin_attn_fwd_kernel, dim3(grid_x(B, Hp, Wp, heads), heads), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t *)qkv, bias, g, (bf16_t *)out, lse);
  return check_launch("swin_attn_fwd");
}

BFHIP_EXPORT int bfhip_swin_attn_bwd(const void *qkv, long long qkv_pitch, const float *bias, const void *out, const void *dout,
                                     const float *lse, int B, int Hp, int Wp, int heads, int shift, float scale, void *dqkv,
                                     float *dbias_partial, int parts, void *stream) {
  BFHIP_REQUIRE(shape_ok(B, Hp, Wp, heads, kWin, kHd, shift), "swin_attn_bwd: unsupported B=%d Hp=%d Wp=%d heads=%d shift=%d", B, Hp, Wp,
                heads, shift);
  BFHIP_REQUIRE(qkv && bias && out && dout && lse && dqkv && dbias_partial, "swin_attn_bwd: null pointer");
  BFHIP_REQUIRE(qkv_pitch >= 3ll * heads * kHd && qkv_pitch % 8 == 0 && ((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                    ((uintptr_t)dout % 16) == 0 && ((uintptr_t)dqkv % 8) == 0,
                "swin_attn_bwd: tensors must be 16-byte aligned, qkv row pitch >= 3C and a multiple of 8");
  BFHIP_REQUIRE(parts == grid_x(B, Hp, Wp, heads), "swin_attn_bwd: parts = %d, bfhip_swin_attn_parts() says %d", parts,
                grid_x(B, Hp, Wp, heads));
  const Geo g = make_geo(B, Hp, Wp, heads, shift, qkv_pitch, scale);
  hipLaunchKernelGGL(swin_attn_bwd_kernel, dim3(parts, heads), dim3(256), 0, (hipStream_t)stream, (const bf16_t *)qkv, bias,
                     (const bf16_t *)out, (const bf16_t *)dout, lse, g, (bf16_t *)dqkv, dbias_partial);
  return check_launch("swin_attn_bwd");
}
