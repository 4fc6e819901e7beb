// spconv_wgrad_tr.hip -- sparse weight gradient on the bf16 matrix cores.
// dW[co][k][ci] = sum over output rows of dout[row][co] * in[pairs[k][row]][ci]  (SubMConv3d / SparseConv3d, spconv's
// (out, kD, kH, kW, in) weight layout): conv2d_wgrad.hip's conv_wgrad_kernel with the rulebook as the gather -- column piece q of a tile is
// (offset k = q*8 / Cin, channels q*8 % Cin ..+8), its source row is pairs[k][row] (-1: no neighbour -> zero piece).  The
// pair index of the NEXT 64-row step is loaded while the current step computes, so the index -> row chain costs one
// round trip per step, not two.  bf16 features in, fp32 accumulate: 16x the matrix rate of the fp32-MFMA kernel in
// spconv_wgrad.hip, which stays for fp32 features.
#include "wgrad_tr.h"

namespace bfhip {
namespace {

struct SpWgradGeom {
  int Cin, Cout, KV, ld, n_rows, nq;  // nq = KV * Cin / 8
  int splits, tiles_co, tiles_k;
  int rows_per_split;                  // multiple of 64
};

__global__ __launch_bounds__(256, 2) void spconv_wgrad_tr_kernel(const bf16_t *__restrict__ in, const bf16_t *__restrict__ dout,
                                                                 const int *__restrict__ pairs, float *__restrict__ slab,
                                                                 SpWgradGeom sg) {
  constexpr int BP = 64, T_BYTES = BP * 256;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  unsigned char *sG = smem, *sX = smem + 2 * T_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tiles = sg.tiles_co * sg.tiles_k;
  const long long lb = xcd_chunked_block(blockIdx.x, (long long)tiles * sg.splits);
  const int split = (int)(lb / tiles), tile = (int)(lb - (long long)split * tiles);
  const int tco = tile / sg.tiles_k, tk = tile - tco * sg.tiles_k;
  const int co0 = tco * 128, q0 = tk * 16;
  const int p_begin = split * sg.rows_per_split;
  const int p_end = min(p_begin + sg.rows_per_split, sg.n_rows);
  const int nsteps = p_end > p_begin ? (p_end - p_begin + BP - 1) / BP : 0;

  const int lrow = lane >> 4, lpos = lane & 15;
  int row[4], pk[4], pci[4], pidx[4];  // this lane's 4 rows, the (offset, channel) of its piece of each, the prefetched pair
  bool qok[4], cok[4];
  int gco[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = w * 16 + i * 4 + lrow;
    const int c = lpos ^ tr_swz(r);
    const int q = q0 + c;
    row[i] = p_begin + r;
    gco[i] = co0 + c * 8;
    cok[i] = gco[i] < sg.Cout;
    qok[i] = q < sg.nq;
    const int k8 = (qok[i] ? q : 0) * 8;
    pk[i] = k8 / sg.Cin;
    pci[i] = k8 - pk[i] * sg.Cin;
    pidx[i] = (qok[i] && row[i] < p_end) ? pairs[(size_t)pk[i] * sg.ld + row[i]] : -1;
  }
  const bf16_t *zsrc = zero_src();
  auto stage = [&](int buf) {  // rows `row[]`, pairs `pidx[]` (already loaded)
    unsigned char *dG = sG + buf * T_BYTES + (w * 16) * 256, *dX = sX + buf * T_BYTES + (w * 16) * 256;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool rok = row[i] < p_end;
      glds16((rok && cok[i]) ? dout + ((size_t)row[i] * sg.Cout + gco[i]) : zsrc, dG + i * 1024);
      glds16(pidx[i] >= 0 ? in + ((size_t)pidx[i] * sg.Cin + pci[i]) : zsrc, dX + i * 1024);
    }
  };
  auto advance = [&]() {  // next step's rows and their pair indices (global loads issued here, consumed by the next stage())
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      row[i] += BP;
      pidx[i] = (qok[i] && row[i] < p_end) ? pairs[(size_t)pk[i] * sg.ld + row[i]] : -1;
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

  if (nsteps > 0) { stage(0); advance(); }
  for (int t = 0; t < nsteps; ++t) {
    const int buf = t & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // step t in LDS, step t + 1's pair indices in registers
    __builtin_amdgcn_s_barrier();
    if (t + 1 < nsteps) { stage(buf ^ 1); advance(); }
    tr_compute_step(sG + buf * T_BYTES, sX + buf * T_BYTES, ad, acc);
  }
  const int Ktot = sg.nq * 8;
  tr_store_slab(slab + (size_t)split * sg.Cout * Ktot, sg.Cout, Ktot, co0, q0, lane, wm, wn, acc);
}

// this unit's own instance of the dense weight gradient's slab sum (conv2d_wgrad.hip), under the same name in a kernel trace
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float *__restrict__ slab, int splits, long long total,
                                                                void *__restrict__ dw, int out_bf16) {
  wgrad_reduce_body(slab, splits, total, dw, out_bf16, blockIdx.x);
}

SpWgradGeom sp_wgrad_geom(int KV, int Cin, int Cout, int ld, int n_rows) {
  SpWgradGeom sg;
  sg.Cin = Cin; sg.Cout = Cout; sg.KV = KV; sg.ld = ld; sg.n_rows = n_rows; sg.nq = KV * Cin / 8;
  sg.tiles_co = ceil_div(Cout, 128);
  sg.tiles_k = ceil_div(KV * Cin, 128);
  // two workgroups per CU, one residency round, at least 4 steps per workgroup
  const SplitPlan p = plan_splits(ceil_div(n_rows, 64), sg.tiles_co * sg.tiles_k, 2 * device_cus(), 4);
  sg.splits = p.splits;
  sg.rows_per_split = (int)p.rows_per_split;
  return sg;
}
}  // namespace

// ---- internal entry points for spconv_wgrad.hip (declared in common.h)
size_t spconv_wgrad_tr_workspace_bytes(int KV, int Cin, int Cout, int n_rows) {
  return align_up((size_t)sp_wgrad_geom(KV, Cin, Cout, 0, n_rows > 0 ? n_rows : 1).splits * Cout * KV * Cin * sizeof(float), 256);
}

bool spconv_wgrad_tr_supported(int KV, int Cin, int Cout) { return Cin % 8 == 0 && Cout % 8 == 0 && Cin >= 8 && KV >= 1; }

int spconv_wgrad_tr(const void *in, const void *dout, const int32_t *pairs, int ld, int KV, int n_rows, int Cin, int Cout,
                    float *dW, void *workspace, size_t workspace_bytes, hipStream_t stream) {
  const SpWgradGeom sg = sp_wgrad_geom(KV, Cin, Cout, ld, n_rows);
  if (workspace_bytes < spconv_wgrad_tr_workspace_bytes(KV, Cin, Cout, n_rows)) { set_error("spconv_wgrad: workspace too small"); return BFHIP_E_WORKSPACE; }
  ProfScope ps_main;
  prof_begin(BFHIP_OP_SPCONV_WGRAD_MAIN, stream, &ps_main);
  launch_big_lds<spconv_wgrad_tr_kernel>(80 * 1024, dim3((unsigned)(sg.tiles_co * sg.tiles_k * sg.splits)), dim3(256), (size_t)4 * 64 * 256,
                                         stream, (const bf16_t *)in, (const bf16_t *)dout, pairs, (float *)workspace, sg);
  prof_end(&ps_main);
  const long long total = (long long)Cout * KV * Cin;
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(ceil_div(total, 1024)), dim3(256), 0, stream, (const float *)workspace, sg.splits,
                     total, (void *)dW, 0);
  return BFHIP_OK;
}

}  // namespace bfhip
