// detection_eval.hip -- the nuScenes detection protocol on the device (gfx950): greedy centre-distance matching of predictions to
// ground truth, the precision / confidence / error curves and the AP and TP scalars, as bevfusion_amd/evaluation.py:
// numpy_detection_eval defines them.  Two launches, whatever the number of samples.
//
//   1. de_match_kernel: one workgroup of 4 waves per (sample, class).  The sample's predictions of the class (at most kMaxPreds
//      per sample) are compacted into LDS in index order and ranked by (score descending, flat index descending) with one
//      all-pairs count per prediction; the sample's GT boxes of the class (at most kMaxGt) are compacted into LDS as float64
//      centres.  Wave w then runs thresholds w, w + 4, ...: it walks the ranked predictions; lane l owns GT l, l + 64, ... and
//      keeps their "taken" bits in ONE REGISTER (bit q for GT l + 64 q), so the bitmask needs no LDS traffic and no ordering
//      between lanes.  Per prediction each lane finds its nearest free GT by strict "<" in ascending GT index, and a butterfly
//      reduction keeps the smaller distance and, on equal distance, the lower GT index.  d < threshold is a match: the owner lane
//      sets its bit, lane 0 writes match[t][p], and for the dist_th_tp threshold the five errors of the pair.
//      d = sqrt(dx dx + dy dy) in float64 on the exactly widened float32 centres, every operation a separate rounding.
//   2. de_curves_kernel: one workgroup per (class, threshold) over the class's predictions in the global (score descending, index
//      descending) order the caller provides.  Phase 1 streams them in tiles of kBlock with an integer scan of the match flags
//      (cumulative TP) and, at dist_th_tp, float64 scans of the four error columns: the cumulative counts, the matched scores and
//      the cumulative error means go to the workspace.  Phase 2: 101 threads binary-search the recall levels in the counts and
//      interpolate precision and confidence (numpy's piecewise-linear rule, one rounding per operation); the error curves are
//      interpolated at those confidences in the matched scores; one thread sums AP, five the TP scalars, sequentially.
// No atomics: every output is a pure function of the inputs, the same bytes on every run.  Offsets, order and class indices
// read from device memory are clamped before they index anything.
#include "common.h"

namespace bfhip {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxPreds = 512;       // predictions per sample (max_boxes_per_sample = 500)
constexpr int kMaxGt = 1024;         // GT boxes per (sample, class)
constexpr int kGtPerLane = kMaxGt / kWave;
constexpr int kMaxThresholds = 8;
constexpr int kMaxClasses = 64;      // one bit per class in the two class masks
constexpr int kBox = 9;              // x, y, z, dx, dy, dz, yaw, vx, vy
constexpr int kLevels = 101;         // recall levels
constexpr int kErr = 5;              // trans, scale, orient, vel, attr
static_assert(kGtPerLane <= 32, "one taken bit per owned GT in a 32-bit register");

struct Thresholds { double v[kMaxThresholds]; };

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }

// rank of a flagged thread among the flagged threads of the block (thread order); *total = their number.  wtot: kWaves ints.
__device__ __forceinline__ int block_rank(bool flag, int *wtot, int *total) {
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const unsigned long long bal = __ballot(flag);
  __syncthreads();  // wtot of the previous use has been read
  if (lane == 0) wtot[wv] = __popcll(bal);
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < kWaves; ++k) {
    if (k < wv) before += wtot[k];
    all += wtot[k];
  }
  *total = all;
  return before + __popcll(bal & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void de_match_kernel(const float *__restrict__ pred, const float *__restrict__ score,
                                                          const int *__restrict__ pred_cls, const int *__restrict__ pred_off,
                                                          long long Np, const float *__restrict__ gt,
                                                          const int *__restrict__ gt_cls, const int *__restrict__ gt_off,
                                                          long long Ng, int C, int T, int tp_idx, Thresholds ths,
                                                          unsigned long long half_period_mask, unsigned long long attr_empty_mask,
                                                          double pi, int *__restrict__ match, double *__restrict__ perr) {
  __shared__ double gxs[kMaxGt], gys[kMaxGt];
  __shared__ int gid[kMaxGt];
  __shared__ double pxs[kMaxPreds], pys[kMaxPreds];
  __shared__ float ps[kMaxPreds];
  __shared__ int pidx[kMaxPreds];
  __shared__ int ord[kMaxPreds];
  __shared__ int wtot[kWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const int s = blockIdx.x / C, c = blockIdx.x % C;

  // the sample's predictions of class c, in index order
  long long p0 = pred_off[s], p1 = pred_off[s + 1];
  p0 = p0 < 0 ? 0 : (p0 > Np ? Np : p0);
  p1 = p1 < p0 ? p0 : (p1 > Np ? Np : p1);
  if (p1 - p0 > kMaxPreds) p1 = p0 + kMaxPreds;
  int n = 0;
  for (long long b = p0; b < p1; b += kBlock) {
    const long long p = b + t;
    const bool mine = p < p1 && pred_cls[p] == c;
    int tot;
    const int r = n + block_rank(mine, wtot, &tot);
    if (mine) {
      pidx[r] = (int)p;
      ps[r] = score[p];
      pxs[r] = (double)pred[p * kBox];
      pys[r] = (double)pred[p * kBox + 1];
      ord[r] = r;  // a valid index even where NaN scores leave two ranks equal
    }
    n += tot;
  }
  if (n == 0) return;  // uniform: nothing of this class to write
  __syncthreads();
  for (int k = t; k < n; k += kBlock) {
    const float sk = ps[k];
    int rank = 0;
    for (int m = 0; m < n; ++m) rank += (ps[m] > sk || (ps[m] == sk && m > k)) ? 1 : 0;  // m > k <=> higher flat index
    if (rank < n) ord[rank] = k;
  }

  // the sample's GT of class c, in index order
  long long g0 = gt_off[s], g1 = gt_off[s + 1];
  g0 = g0 < 0 ? 0 : (g0 > Ng ? Ng : g0);
  g1 = g1 < g0 ? g0 : (g1 > Ng ? Ng : g1);
  int m = 0;
  for (long long b = g0; b < g1; b += kBlock) {
    const long long g = b + t;
    const bool mine = g < g1 && gt_cls[g] == c;
    int tot;
    const int r = m + block_rank(mine, wtot, &tot);
    if (mine && r < kMaxGt) {
      gid[r] = (int)g;
      gxs[r] = (double)gt[g * kBox];
      gys[r] = (double)gt[g * kBox + 1];
    }
    m += tot;
  }
  if (m > kMaxGt) m = kMaxGt;
  __syncthreads();

  for (int ti = wv; ti < T; ti += kWaves) {
    const double th = ths.v[ti];
    unsigned int taken = 0u;
    for (int r = 0; r < n; ++r) {
      const int k = ord[r];
      const double px = pxs[k], py = pys[k];
      double best = __longlong_as_double(0x7ff0000000000000ll);  // +inf
      int bj = 0x7fffffff;
      for (int q = 0; q < kGtPerLane; ++q) {
        const int j = lane + q * kWave;
        if (j >= m) break;
        if ((taken >> q) & 1u) continue;
        const double dx = __dsub_rn(gxs[j], px), dy = __dsub_rn(gys[j], py);
        const double d = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
        if (d < best) best = d, bj = j;
      }
      for (int o = kWave / 2; o > 0; o >>= 1) {
        const double od = __shfl_xor(best, o);
        const int oj = __shfl_xor(bj, o);
        if (od < best || (od == best && oj < bj)) best = od, bj = oj;
      }
      const bool hit = best < th;  // wave-uniform; false when no GT is free (best = +inf) or the distance is NaN
      if (hit && (bj & (kWave - 1)) == lane) taken |= 1u << (bj / kWave);
      if (lane == 0) {
        const long long p = pidx[k];
        match[(long long)ti * Np + p] = hit ? gid[bj] : -1;
        if (ti == tp_idx) {
          double *e = perr + p * kErr;
          if (hit) {
            const float *pb = pred + p * kBox;
            const float *gb = gt + (long long)gid[bj] * kBox;
            const double pdx = pb[3], pdy = pb[4], pdz = pb[5], gdx = gb[3], gdy = gb[4], gdz = gb[5];
            const double inter = __dmul_rn(__dmul_rn(fmin(pdx, gdx), fmin(pdy, gdy)), fmin(pdz, gdz));
            const double vp = __dmul_rn(__dmul_rn(pdx, pdy), pdz), vg = __dmul_rn(__dmul_rn(gdx, gdy), gdz);
            const double uni = __dsub_rn(__dadd_rn(vg, vp), inter);
            const double period = ((half_period_mask >> c) & 1ull) ? pi : __dmul_rn(2.0, pi);
            const double half = __ddiv_rn(period, 2.0);
            const double a = __dadd_rn(__dsub_rn((double)gb[6], (double)pb[6]), half);
            double r_ = fmod(a, period);  // exact; floored as Python's %: the sign of the divisor
            if (r_ != 0.0 && r_ < 0.0) r_ = __dadd_rn(r_, period);
            double diff = __dsub_rn(r_, half);
            if (diff > pi) diff = __dsub_rn(diff, __dmul_rn(2.0, pi));
            const double dvx = __dsub_rn((double)gb[7], (double)pb[7]), dvy = __dsub_rn((double)gb[8], (double)pb[8]);
            e[0] = best;
            e[1] = __dsub_rn(1.0, __ddiv_rn(inter, uni));
            e[2] = fabs(diff);
            e[3] = __dsqrt_rn(__dadd_rn(__dmul_rn(dvx, dvx), __dmul_rn(dvy, dvy)));
            e[4] = ((attr_empty_mask >> c) & 1ull) ? qnan() : 0.0;
          } else {
            for (int q = 0; q < kErr; ++q) e[q] = qnan();
          }
        }
      }
    }
  }
}

struct CurveOut {
  double *prec, *conf, *err, *ap, *tp;  // [C,T,101] [C,T,101] [C,5,101] [C,T] [C,5]
  int *mri;                             // [C]
};

// numpy's interp at one x over ascending xp(0..n-1) with values fp: X and F are callables on an index
template <typename X, typename F>
__device__ __forceinline__ double interp_at(double x, int j, int n, X xp, F fp) {
  const double xj = xp(j), fj = fp(j);
  if (x == xj || j == n - 1) return fj;
  const double slope = __ddiv_rn(__dsub_rn(fp(j + 1), fj), __dsub_rn(xp(j + 1), xj));
  return __dadd_rn(__dmul_rn(slope, __dsub_rn(x, xj)), fj);
}

__global__ __launch_bounds__(kBlock) void de_curves_kernel(const float *__restrict__ score, const int *__restrict__ order,
                                                           const int *__restrict__ cls_off, const int *__restrict__ match,
                                                           const double *__restrict__ perr, long long Np, int T, int tp_idx,
                                                           const int *__restrict__ npos_g, const double *__restrict__ levels,
                                                           double min_precision, int first, unsigned long long attr_empty_mask,
                                                           int *__restrict__ tpc_g, double *__restrict__ ms_g,
                                                           double *__restrict__ cm_g, CurveOut out) {
  __shared__ int wti[kWaves];
  __shared__ double wtd[4][kWaves];
  __shared__ double sp[kLevels], sc[kLevels];
  __shared__ double se[kErr][kLevels];
  const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const int c = blockIdx.x / T, ti = blockIdx.x % T;
  const bool is_tp = ti == tp_idx;
  long long lo = cls_off[c], hi = cls_off[c + 1];
  lo = lo < 0 ? 0 : (lo > Np ? Np : lo);
  hi = hi < lo ? lo : (hi > Np ? Np : hi);
  const int n = (int)(hi - lo);
  const int npos = npos_g[c];
  int *tpc = tpc_g + (long long)ti * Np + lo;  // cumulative TP of this (class, threshold)
  double *ms = ms_g + lo;                      // matched scores, match order (dist_th_tp only)
  const int *ord = order + lo;

  // phase 1: scans over the ordered predictions
  int carry = 0;
  double dcarry[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < n; b += kBlock) {
    const int j = b + t;
    long long p = j < n ? ord[j] : -1;
    if (p >= Np) p = -1;
    const bool flag = p >= 0 && match[(long long)ti * Np + p] >= 0;
    int incl = flag ? 1 : 0;
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    if (is_tp && flag)
      for (int q = 0; q < 4; ++q) e[q] = perr[p * kErr + q];
    for (int o = 1; o < kWave; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (is_tp)
      for (int q = 0; q < 4; ++q)
        for (int o = 1; o < kWave; o <<= 1) {
          const double up = __shfl_up(e[q], o);
          if (lane >= o) e[q] = __dadd_rn(e[q], up);
        }
    __syncthreads();  // the totals of the previous tile have been read
    if (lane == kWave - 1) {
      wti[wv] = incl;
      if (is_tp)
        for (int q = 0; q < 4; ++q) wtd[q][wv] = e[q];
    }
    __syncthreads();
    int before = carry, all = carry;
    for (int k = 0; k < kWaves; ++k) {
      if (k < wv) before += wti[k];
      all += wti[k];
    }
    const int tp_incl = before + incl;
    if (j < n) tpc[j] = tp_incl;
    if (is_tp) {
      for (int q = 0; q < 4; ++q) {
        double bq = dcarry[q], aq = dcarry[q];
        for (int k = 0; k < kWaves; ++k) {
          if (k < wv) bq = __dadd_rn(bq, wtd[q][k]);
          aq = __dadd_rn(aq, wtd[q][k]);
        }
        if (flag) cm_g[(long long)q * Np + lo + (tp_incl - 1)] = __ddiv_rn(__dadd_rn(bq, e[q]), (double)tp_incl);
        dcarry[q] = aq;
      }
      if (flag) ms[tp_incl - 1] = (double)score[p];
    }
    carry = all;
  }
  const int M = carry;
  __threadfence_block();
  __syncthreads();

  double *o_prec = out.prec + ((long long)c * T + ti) * kLevels;
  double *o_conf = out.conf + ((long long)c * T + ti) * kLevels;
  double *o_err = out.err + (long long)c * kErr * kLevels;
  if (npos <= 0 || M == 0) {  // the empty curve
    if (t < kLevels) o_prec[t] = 0.0, o_conf[t] = 0.0;
    if (is_tp) {
      for (int w = t; w < kErr * kLevels; w += kBlock) o_err[w] = 1.0;
      if (t < kErr) out.tp[c * kErr + t] = 1.0;
      if (t == 0) out.mri[c] = 0;
    }
    if (t == 0) out.ap[c * T + ti] = 0.0;
    return;
  }

  // phase 2: precision and confidence at the recall levels
  const double dn = (double)npos;
  auto rec = [&](int j) { return __ddiv_rn((double)tpc[j], dn); };
  auto prec = [&](int j) { return __ddiv_rn((double)tpc[j], (double)(j + 1)); };
  auto conf = [&](int j) {
    const long long p = ord[j];
    return p >= 0 && p < Np ? (double)score[p] : 0.0;
  };
  if (t < kLevels) {
    const double x = levels[t];
    double vp, vc;
    if (x > rec(n - 1)) {
      vp = 0.0, vc = 0.0;
    } else if (x < rec(0)) {
      vp = prec(0), vc = conf(0);
    } else {
      int a = 0, b = n;  // the number of j with rec(j) <= x
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (rec(mid) <= x) a = mid + 1; else b = mid;
      }
      vp = interp_at(x, a - 1, n, rec, prec);
      vc = interp_at(x, a - 1, n, rec, conf);
    }
    sp[t] = vp, sc[t] = vc;
    o_prec[t] = vp, o_conf[t] = vc;
  }
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int i = first; i < kLevels; ++i) {
      const double v = __dsub_rn(sp[i], min_precision);
      sum = __dadd_rn(sum, v < 0.0 ? 0.0 : v);
    }
    out.ap[c * T + ti] = __ddiv_rn(__ddiv_rn(sum, (double)(kLevels - first)), __dsub_rn(1.0, min_precision));
  }
  if (!is_tp) return;

  // the error curves: numpy's interp of the cumulative means over the ASCENDING (reversed) matched scores, at the confidences
  for (int w = t; w < kErr * kLevels; w += kBlock) {
    const int q = w / kLevels, i = w % kLevels;
    double v;
    if (q == 4) {
      v = ((attr_empty_mask >> c) & 1ull) ? 1.0 : 0.0;  // the mean of zeros; of nothing but NaN: ones
    } else {
      const double *cm = cm_g + (long long)q * Np + lo;
      auto xa = [&](int j) { return ms[M - 1 - j]; };
      auto fa = [&](int j) { return cm[M - 1 - j]; };
      const double x = sc[i];
      if (x > xa(M - 1)) {
        v = fa(M - 1);
      } else if (x < xa(0)) {
        v = fa(0);
      } else {
        int a = 0, b = M;
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (xa(mid) <= x) a = mid + 1; else b = mid;
        }
        v = interp_at(x, a - 1, M, xa, fa);
      }
    }
    se[q][i] = v;
    o_err[w] = v;
  }
  __syncthreads();
  if (t < kErr) {
    int last = 0;
    for (int i = 0; i < kLevels; ++i)
      if (sc[i] != 0.0) last = i;
    double v = 1.0;
    if (last >= first) {
      double sum = 0.0;
      for (int i = first; i <= last; ++i) sum = __dadd_rn(sum, se[t][i]);
      v = __ddiv_rn(sum, (double)(last - first + 1));
    }
    out.tp[c * kErr + t] = v;
    if (t == 0) out.mri[c] = last;
  }
}

size_t curves_ws_bytes(long long Np, int T) {
  return align_up((size_t)T * (size_t)Np * sizeof(int), 256) + 5 * align_up((size_t)Np * sizeof(double), 256);
}

}  // namespace
}  // namespace bfhip

using namespace bfhip;

BFHIP_EXPORT int bfhip_detection_eval_max_preds(void) { return kMaxPreds; }
BFHIP_EXPORT int bfhip_detection_eval_max_gt(void) { return kMaxGt; }
BFHIP_EXPORT int bfhip_detection_eval_max_thresholds(void) { return kMaxThresholds; }
BFHIP_EXPORT int bfhip_detection_eval_max_classes(void) { return kMaxClasses; }

BFHIP_EXPORT int bfhip_detection_match(const float *pred, const float *score, const int32_t *pred_cls, const int32_t *pred_off,
                                       long long n_pred, const float *gt, const int32_t *gt_cls, const int32_t *gt_off,
                                       long long n_gt, int n_samples, int n_classes, const double *dist_ths, int n_ths, int tp_index,
                                       uint64_t half_period_mask, uint64_t attr_empty_mask, int32_t *match, double *pred_err,
                                       void *stream) {
  BFHIP_REQUIRE(n_pred >= 0 && n_pred < 0x80000000ll, "detection_match: %lld predictions (0 .. 2^31 - 1)", n_pred);
  BFHIP_REQUIRE(n_gt >= 0 && n_gt < 0x80000000ll, "detection_match: %lld GT boxes (0 .. 2^31 - 1)", n_gt);
  BFHIP_REQUIRE(n_samples >= 0 && n_classes >= 1 && n_classes <= kMaxClasses, "detection_match: %d samples, %d classes (1 .. %d)",
                n_samples, n_classes, kMaxClasses);
  BFHIP_REQUIRE((long long)n_samples * n_classes < 0x80000000ll, "detection_match: %d samples x %d classes (below 2^31)", n_samples,
                n_classes);
  BFHIP_REQUIRE(dist_ths && n_ths >= 1 && n_ths <= kMaxThresholds, "detection_match: %d thresholds (1 .. %d), dist_ths %s", n_ths,
                kMaxThresholds, dist_ths ? "given" : "NULL");
  BFHIP_REQUIRE(tp_index >= 0 && tp_index < n_ths, "detection_match: tp_index=%d of %d thresholds", tp_index, n_ths);
  BFHIP_REQUIRE(n_samples == 0 || (pred_off && gt_off), "detection_match: pred_off or gt_off is NULL");
  BFHIP_REQUIRE(n_pred == 0 || (pred && score && pred_cls && match && pred_err), "detection_match: a prediction array is NULL");
  BFHIP_REQUIRE(n_gt == 0 || (gt && gt_cls), "detection_match: a GT array is NULL");
  BFHIP_REQUIRE((((uintptr_t)pred | (uintptr_t)score | (uintptr_t)pred_cls | (uintptr_t)pred_off | (uintptr_t)gt | (uintptr_t)gt_cls |
                  (uintptr_t)gt_off | (uintptr_t)match) & 3) == 0, "detection_match: an array is not 4-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)pred_err & 7) == 0, "detection_match: pred_err not 8-byte aligned");
  if (n_samples == 0 || n_pred == 0) return BFHIP_OK;
  Thresholds ths;
  for (int i = 0; i < kMaxThresholds; ++i) ths.v[i] = i < n_ths ? dist_ths[i] : 0.0;
  hipLaunchKernelGGL(de_match_kernel, dim3((unsigned)(n_samples * n_classes)), dim3(kBlock), 0, (hipStream_t)stream, pred, score,
                     pred_cls, pred_off, n_pred, gt, gt_cls, gt_off, n_gt, n_classes, n_ths, tp_index, ths,
                     (unsigned long long)half_period_mask, (unsigned long long)attr_empty_mask, 3.141592653589793, match, pred_err);
  return check_launch("detection_match");
}

BFHIP_EXPORT size_t bfhip_detection_curves_workspace_bytes(long long n_pred, int n_ths) {
  if (n_pred < 0 || n_pred >= 0x80000000ll || n_ths < 1 || n_ths > kMaxThresholds) return 0;
  return curves_ws_bytes(n_pred, n_ths);
}

BFHIP_EXPORT int bfhip_detection_curves(const float *score, const int32_t *order, const int32_t *cls_off, const int32_t *match,
                                        const double *pred_err, long long n_pred, int n_classes, int n_ths, int tp_index,
                                        const int32_t *npos, const double *levels, double min_precision, int first_level,
                                        uint64_t attr_empty_mask, double *precision, double *confidence, double *err_curves,
                                        double *ap, double *tp_err, int32_t *max_recall_ind, void *workspace,
                                        size_t workspace_bytes, void *stream) {
  BFHIP_REQUIRE(n_pred >= 1 && n_pred < 0x80000000ll, "detection_curves: %lld predictions (1 .. 2^31 - 1)", n_pred);
  BFHIP_REQUIRE(n_classes >= 1 && n_classes <= kMaxClasses, "detection_curves: %d classes (1 .. %d)", n_classes, kMaxClasses);
  BFHIP_REQUIRE(n_ths >= 1 && n_ths <= kMaxThresholds, "detection_curves: %d thresholds (1 .. %d)", n_ths, kMaxThresholds);
  BFHIP_REQUIRE(tp_index >= 0 && tp_index < n_ths, "detection_curves: tp_index=%d of %d thresholds", tp_index, n_ths);
  BFHIP_REQUIRE(first_level >= 0 && first_level < kLevels, "detection_curves: first_level=%d (0 .. %d)", first_level, kLevels - 1);
  BFHIP_REQUIRE(score && order && cls_off && match && pred_err && npos && levels, "detection_curves: an input array is NULL");
  BFHIP_REQUIRE(precision && confidence && err_curves && ap && tp_err && max_recall_ind, "detection_curves: an output array is NULL");
  BFHIP_REQUIRE((((uintptr_t)score | (uintptr_t)order | (uintptr_t)cls_off | (uintptr_t)match | (uintptr_t)npos |
                  (uintptr_t)max_recall_ind) & 3) == 0, "detection_curves: an array is not 4-byte aligned");
  BFHIP_REQUIRE((((uintptr_t)pred_err | (uintptr_t)levels | (uintptr_t)precision | (uintptr_t)confidence | (uintptr_t)err_curves |
                  (uintptr_t)ap | (uintptr_t)tp_err) & 7) == 0, "detection_curves: a float64 array is not 8-byte aligned");
  BFHIP_REQUIRE(((uintptr_t)workspace & 255) == 0, "detection_curves: workspace not 256-byte aligned");
  const size_t need = curves_ws_bytes(n_pred, n_ths);
  BFHIP_REQUIRE_WORKSPACE(workspace, workspace_bytes, need, "detection_curves");
  Workspace ws(workspace, workspace_bytes);
  int *tpc = ws.take<int>((size_t)n_ths * (size_t)n_pred);
  double *ms = ws.take<double>((size_t)n_pred);
  double *cm = ws.take<double>(4 * (size_t)n_pred);
  BFHIP_REQUIRE(tpc && ms && cm, "detection_curves: workspace layout");
  CurveOut out{precision, confidence, err_curves, ap, tp_err, max_recall_ind};
  hipLaunchKernelGGL(de_curves_kernel, dim3((unsigned)(n_classes * n_ths)), dim3(kBlock), 0, (hipStream_t)stream, score, order,
                     cls_off, match, pred_err, n_pred, n_ths, tp_index, npos, levels, min_precision, first_level,
                     (unsigned long long)attr_empty_mask, tpc, ms, cm, out);
  return check_launch("detection_curves");
}
