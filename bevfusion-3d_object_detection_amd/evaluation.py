"""The step after predict(): the reference's `val_evaluator = dict(type='NuScenesCustomMetric', ...)` (projects/BEVFusion/
configs/custom_data/lidar_custom.py:264-270, projects/BEVFusion/evaluation/) -- boxes, scores and labels in, AP, mATE / mASE /
mAOE / mAVE / mAAE and NDS out.

    metrics = detection_eval(preds, gts, cfg, classes)

`preds`: per sample, in evaluation order, (boxes float32 [n, 7 or 9], scores float32 [n], labels int [n]) -- tensors (any
device) or arrays, boxes in LiDAR convention (x, y, z of the bottom centre, dx, dy, dz, yaw[, vx, vy]), what predict() returns.
`gts`: per sample (bbox_3d [m, 7] with the GRAVITY centre, bbox_label_3d [m]) as the infos carry them.  `cfg`: a DetectionConfig;
`classes`: the data set's class names (label -> name).  The result is the devkit's `DetectionMetrics.serialize()` dict
(label_aps, mean_dist_aps, mean_ap, label_tp_errors, tp_errors, tp_scores, nd_score, cfg) plus the raw tables: match, pred_errors,
precision, confidence, err_curves, aps, tp_table, max_recall_ind.

The reference keeps boxes in the LiDAR frame (the global transform and the class-range filter are commented out, nuscenes_
custom_metric.py:686-688, 780-782; its evaluator stops before the stock filtering, functional/nuscenes_utils/eval.py:139-179) and
then calls the nuScenes devkit's evaluate().  The devkit is not part of the reference tree; its protocol (accumulate, calc_ap,
calc_tp, the detection_cvpr_2019 settings) is restated here in float64 numpy, and THAT RESTATEMENT, `numpy_detection_eval`, IS
THE SPECIFICATION.  Parity with the devkit's own numbers is by construction of the restatement and is unmeasured.

The protocol.  Centres: predictions (x, y, fl32(z + fl32(dz 0.5))); GT goes through the two float32 steps of
LiDARInstance3DBoxes(origin=(0.5, 0.5, 0.5)).gravity_center: z_b = fl32(z + fl32(dz (-0.5))), z_c = fl32(z_b + fl32(dz 0.5)); GT
velocity is (0, 0) (nuscenes_custom_metric.py:739-761).  A GT label outside [0, len(classes)) is dropped (the reference's list
index would wrap -1 to the last class).  Everything after is float64 on those float32 values, one IEEE operation per product,
sum, quotient and sqrt.  Per class c of cfg.class_names and threshold t: the predictions of c over all samples by score
descending, at equal score the HIGHER flat index first (the devkit's sorted((score, i))[::-1]); each takes, among the not yet taken
GT of c in its own sample, the one with the smallest d = sqrt(dx dx + dy dy) (the first on a tie) iff d < t.  At t = dist_th_tp a
match has the errors (TP_METRICS order) trans = d; scale = 1 - I / (Va + Vb - I), I = min(dx) min(dy) min(dz); orient = |diff|,
diff = ((yaw_gt - yaw_pred + period / 2) mod period) - period / 2 with the floored modulo, diff -= 2 pi if diff > pi, period pi
for 'barrier' and 2 pi otherwise -- the yaw is used directly, the reference goes yaw -> quaternion -> yaw (a departure of
rounding size); vel = sqrt(dvx^2 + dvy^2); attr = 0 where the class's DefaultAttribute is non-empty, NaN where it is ''.  Curves
per (c, t): prec = tp / (tp + fp), rec = tp / npos over the ordered predictions, precision = interp(linspace(0, 1, 101), rec, prec,
right=0), confidence likewise of the scores; the error curves are the cumulative means of the matched errors, interpolated at
the confidences over the matched scores; with npos = 0 or no match the empty curve (precision, confidence 0, errors 1).  AP =
mean(max(precision[11:] - min_precision, 0)) / (1 - min_precision), summed in index order; a TP metric is the mean of its curve
over [11, last non-zero confidence], or 1.  mean_ap averages over cfg.class_names (classes without GT count 0); nd_score =
(w mean_ap + sum(1 - min(1, tp_error))) / (w + 5).  More than max_boxes_per_sample predictions in a sample, a non-finite score or
box value, or a prediction label outside [0, len(classes)) raise ValueError; a class missing from DefaultAttribute raises KeyError.

On the GPU the work is csrc/detection_eval.hip: bfhip_detection_match (all samples x classes x thresholds in one launch) and
bfhip_detection_curves (one workgroup per (class, threshold)), with the global order from two stable torch sorts on the device.
A fixed number of launches, no atomics, and no host read before the final small tables.  match, pred_errors, precision,
confidence, aps and max_recall_ind are bit for bit the specification's; the cumulative error means are sums whose order differs
from numpy's sequential one, so err_curves and the TP scalars agree to 2 (n - 1) 2^-53 relative, n the matched count.  At most
max_preds() predictions per sample and max_gt() GT boxes per (sample, class); above that, for CPU tensors or arrays, and with
BFHIP_DETECTION_EVAL=0 the specification runs, same results.  PATHS counts the calls each way took.

BFHIP_DETECTION_EVAL ships on (measured with tools/detection_eval_micro.py: DESIGN.md section 6).
"""
import json
import math
import os
import pickle

import numpy as np
import torch

from . import _lib
from .registry import METRICS

ENABLED = os.environ.get("BFHIP_DETECTION_EVAL", "1") != "0"
PATHS = {"kernel": 0, "torch": 0}  # calls taken by each path (tests, tools)

TP_METRICS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")
N_LEVELS = 101

DEFAULT_ATTRIBUTE = {
    "car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked", "truck": "vehicle.parked",
    "bus": "vehicle.moving", "motorcycle": "cycle.without_rider", "construction_vehicle": "vehicle.parked",
    "bicycle": "cycle.without_rider", "barrier": "", "traffic_cone": "",
}
ERR_NAME_MAPPING = {"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE", "attr_err": "mAAE"}


class DetectionConfig:
    """The evaluation settings (functional/nuscenes_utils/eval.py:42-105).  class_range is carried, not applied."""

    def __init__(self, class_names, class_range, dist_fcn, dist_ths, dist_th_tp, min_recall, min_precision, max_boxes_per_sample,
                 mean_ap_weight):
        assert dist_th_tp in dist_ths, "dist_th_tp must be in set of dist_ths."
        self.class_range = class_range
        self.dist_fcn = dist_fcn
        self.dist_ths = dist_ths
        self.dist_th_tp = dist_th_tp
        self.min_recall = min_recall
        self.min_precision = min_precision
        self.max_boxes_per_sample = max_boxes_per_sample
        self.mean_ap_weight = mean_ap_weight
        self.class_names = class_names

    def __eq__(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.serialize())

    def serialize(self):
        return {k: getattr(self, k) for k in ("class_names", "class_range", "dist_fcn", "dist_ths", "dist_th_tp", "min_recall",
                                              "min_precision", "max_boxes_per_sample", "mean_ap_weight")}

    @classmethod
    def deserialize(cls, content):
        return cls(content["class_names"], content["class_range"], content["dist_fcn"], content["dist_ths"], content["dist_th_tp"],
                   content["min_recall"], content["min_precision"], content["max_boxes_per_sample"], content["mean_ap_weight"])


def config_factory(name="detection_cvpr_2019", class_names=None):
    """The named settings; class_names: average over these classes instead of the keys of class_range."""
    if name != "detection_cvpr_2019":
        raise ValueError("unknown evaluation configuration %r" % (name,))
    class_range = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40, "motorcycle": 40,
                   "bicycle": 40, "traffic_cone": 30, "barrier": 30}
    return DetectionConfig(list(class_names) if class_names is not None else list(class_range), class_range, "center_distance",
                           [0.5, 1.0, 2.0, 4.0], 2.0, 0.1, 0.1, 500, 5)


# ---------------------------------------------------------------------------------------------------------------- packing
def _np(x):
    x = getattr(x, "tensor", x)
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _unpack_pred(p):
    if isinstance(p, dict):
        p = p.get("pred_instances_3d", p)
        return p["bboxes_3d"], p["scores_3d"], p["labels_3d"]
    return p


def gt_lidar_boxes(bbox_3d):
    """float32 [m, 9] (x, y, z_centre, dx, dy, dz, yaw, 0, 0) of the infos' gravity-centre boxes [m, 7+]: the two float32 steps of
    LiDARInstance3DBoxes(origin=(0.5, 0.5, 0.5)) and .gravity_center on z."""
    b = np.asarray(bbox_3d, dtype=np.float64).reshape(-1, np.shape(bbox_3d)[-1] if np.size(bbox_3d) else 7)[:, :7].astype(np.float32)
    out = np.zeros((b.shape[0], 9), np.float32)
    out[:, :7] = b
    z_b = b[:, 2] + b[:, 5] * np.float32(-0.5)
    out[:, 2] = z_b + b[:, 5] * np.float32(0.5)
    return out


def pred_lidar_boxes(boxes):
    """float32 [n, 9] (x, y, z_centre, dx, dy, dz, yaw, vx, vy) of predictions [n, 7 or 9] with the bottom centre."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, np.shape(boxes)[-1] if np.size(boxes) else 9)
    if b.shape[1] not in (7, 9):
        raise ValueError("prediction boxes must be [n, 7 or 9], got %s" % (b.shape,))
    out = np.zeros((b.shape[0], 9), np.float32)
    out[:, :b.shape[1]] = b
    out[:, 2] = b[:, 2] + b[:, 5] * np.float32(0.5)
    return out


def _class_tables(cfg, classes):
    """(lut int32 [len(classes)]: label -> index into cfg.class_names or -1, period float64 [C], attr_empty bool [C])."""
    names = list(cfg.class_names)
    for n in list(classes) + names:
        DEFAULT_ATTRIBUTE[n]  # KeyError for a class without a default attribute, as the reference's formatting raises
    lut = np.array([names.index(n) if n in names else -1 for n in classes], np.int32).reshape(-1)
    period = np.array([np.pi if n == "barrier" else 2 * np.pi for n in names], np.float64)
    attr_empty = np.array([DEFAULT_ATTRIBUTE[n] == "" for n in names], bool)
    return lut, period, attr_empty


def pack_gt(gts, cfg, classes):
    """(G float32 [Ng, 9], g_cls int32 [Ng], g_off int32 [S + 1]) on the host; labels outside [0, len(classes)) are dropped."""
    lut, _, _ = _class_tables(cfg, classes)
    boxes, cls, off = [], [], [0]
    for b, l in gts:
        l = _np(l).astype(np.int64).reshape(-1)
        b = gt_lidar_boxes(_np(b)) if l.size else np.zeros((0, 9), np.float32)
        keep = (l >= 0) & (l < len(lut))
        boxes.append(b[keep])
        cls.append(lut[l[keep]] if len(lut) else np.zeros(0, np.int32))
        off.append(off[-1] + int(keep.sum()))
    G = np.concatenate(boxes, 0) if boxes else np.zeros((0, 9), np.float32)
    return np.ascontiguousarray(G), (np.concatenate(cls) if cls else np.zeros(0, np.int32)).astype(np.int32), np.array(off, np.int32)


def _check_counts(preds, gts, cfg):
    if len(preds) != len(gts):
        raise ValueError("%d samples of predictions, %d of ground truth" % (len(preds), len(gts)))
    for i, p in enumerate(preds):
        n = int(p[1].shape[0])
        if n > cfg.max_boxes_per_sample:
            raise ValueError("Error: Only <= %d boxes per sample allowed! (sample %d has %d)" % (cfg.max_boxes_per_sample, i, n))


def pack_preds_numpy(preds, cfg, classes):
    """(P float32 [Np, 9], scores float32 [Np], p_cls int32 [Np], p_off int32 [S + 1]) on the host."""
    lut, _, _ = _class_tables(cfg, classes)
    boxes, scores, cls, off = [], [], [], [0]
    for b, s, l in preds:
        s = _np(s).astype(np.float32).reshape(-1)
        l = _np(l).astype(np.int64).reshape(-1)
        b = pred_lidar_boxes(_np(b)) if s.size else np.zeros((0, 9), np.float32)
        if not (np.isfinite(b).all() and np.isfinite(s).all()):
            raise ValueError("detection_eval: a non-finite score or box value")
        if ((l < 0) | (l >= len(lut))).any():
            raise ValueError("detection_eval: a prediction label outside [0, %d)" % len(lut))
        boxes.append(b), scores.append(s), cls.append(lut[l]), off.append(off[-1] + s.size)
    cat = lambda xs, shape, dt: np.ascontiguousarray(np.concatenate(xs, 0)) if xs else np.zeros(shape, dt)  # noqa: E731
    return cat(boxes, (0, 9), np.float32), cat(scores, (0,), np.float32), cat(cls, (0,), np.int32).astype(np.int32), \
        np.array(off, np.int32)


# ------------------------------------------------------------------------------------------------------- the specification
def interp(x, xp, fp, left=None, right=None):
    """numpy's piecewise-linear rule with explicit operations: below xp[0] `left` (fp[0]), above xp[-1] `right` (fp[-1]);
    otherwise with j the last index with xp[j] <= x: fp[j] if x == xp[j] or j is the last, else
    (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]) * (x - xp[j]) + fp[j]."""
    x, xp, fp = np.asarray(x, np.float64), np.asarray(xp, np.float64), np.asarray(fp, np.float64)
    n = xp.shape[0]
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, n - 1)
    j1 = np.minimum(j + 1, n - 1)
    with np.errstate(all="ignore"):
        slope = (fp[j1] - fp[j]) / (xp[j1] - xp[j])
        lin = slope * (x - xp[j]) + fp[j]
    out = np.where((x == xp[j]) | (j == n - 1), fp[j], lin)
    out = np.where(x < xp[0], fp[0] if left is None else left, out)
    return np.where(x > xp[-1], fp[-1] if right is None else right, out)


def _seq_sum(values):
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def floored_mod(a, b):
    """Python's a % b for float64 arrays (b > 0): the exact fmod, moved to the divisor's sign."""
    r = np.fmod(a, b)
    return np.where((r != 0) & (r < 0), r + b, r)


def match_errors(P, G, period, attr_empty, d):
    """float64 [k, 5] (TP_METRICS order) of k matched pairs: rows P, G float32 [k, 9], their classes' period and attr_empty, the
    matching distance d."""
    P, G = P.astype(np.float64), G.astype(np.float64)
    inter = np.minimum(P[:, 3], G[:, 3]) * np.minimum(P[:, 4], G[:, 4]) * np.minimum(P[:, 5], G[:, 5])
    vp, vg = P[:, 3] * P[:, 4] * P[:, 5], G[:, 3] * G[:, 4] * G[:, 5]
    scale = 1.0 - inter / ((vg + vp) - inter)
    half = period / 2.0
    diff = floored_mod((G[:, 6] - P[:, 6]) + half, period) - half
    diff = np.where(diff > np.pi, diff - 2.0 * np.pi, diff)
    dvx, dvy = G[:, 7] - P[:, 7], G[:, 8] - P[:, 8]
    vel = np.sqrt(dvx * dvx + dvy * dvy)
    return np.stack([d, scale, np.abs(diff), vel, np.where(attr_empty, np.nan, 0.0)], 1)


def numpy_match(P, scores, p_cls, p_off, G, g_cls, g_off, cfg, period, attr_empty):
    """(match int32 [T, Np], pred_errors float64 [Np, 5]) of the packed arrays: the matching of the module docstring."""
    T, Np, C = len(cfg.dist_ths), P.shape[0], len(cfg.class_names)
    tp_idx = list(cfg.dist_ths).index(cfg.dist_th_tp)
    match = np.full((T, Np), -1, np.int32)
    errors = np.full((Np, 5), np.nan, np.float64)
    px, py, gx, gy = (a.astype(np.float64) for a in (P[:, 0], P[:, 1], G[:, 0], G[:, 1]))
    for s in range(len(p_off) - 1):
        p0, p1, g0, g1 = int(p_off[s]), int(p_off[s + 1]), int(g_off[s]), int(g_off[s + 1])
        pc, gc = p_cls[p0:p1], g_cls[g0:g1]
        for c in np.unique(pc):
            if c < 0 or c >= C:
                continue
            gi = g0 + np.flatnonzero(gc == c)
            if gi.size == 0:
                continue
            pi = p0 + np.flatnonzero(pc == c)
            pi = pi[np.lexsort((-pi, -scores[pi].astype(np.float64)))]  # score descending, then index descending
            dx, dy = gx[gi][None, :] - px[pi][:, None], gy[gi][None, :] - py[pi][:, None]
            D = np.sqrt(dx * dx + dy * dy)
            for t, th in enumerate(cfg.dist_ths):
                free = np.ones(gi.size, bool)
                for r in range(pi.size):
                    row = np.where(free, D[r], np.inf)
                    j = int(np.argmin(row))  # the first of equal minima
                    if row[j] < th:
                        free[j] = False
                        match[t, pi[r]] = gi[j]
                        if t == tp_idx:
                            errors[pi[r], 0] = row[j]
    m = np.flatnonzero(match[tp_idx] >= 0)
    if m.size:
        c = p_cls[m]
        errors[m] = match_errors(P[m], G[match[tp_idx][m]], period[c], attr_empty[c], errors[m, 0])
    return match, errors


def global_order(scores, p_cls, C):
    """(order [Np], cls_off [C + 1]): the flat prediction indices by (class ascending, score descending, index descending), the
    ignored class (-1) last, and each class's first position."""
    key = np.where((p_cls < 0) | (p_cls >= C), C, p_cls)
    idx = np.arange(scores.shape[0])
    order = np.lexsort((-idx, -scores.astype(np.float64), key))
    return order.astype(np.int32), np.searchsorted(key[order], np.arange(C + 1)).astype(np.int32)


def numpy_curves(scores, order, cls_off, match, errors, npos, cfg, attr_empty):
    """The curve tables of the module docstring: dict(precision, confidence [C, T, 101], err_curves [C, 5, 101], aps [C, T],
    tp_table [C, 5], max_recall_ind [C])."""
    C, T = len(cfg.class_names), len(cfg.dist_ths)
    tp_idx = list(cfg.dist_ths).index(cfg.dist_th_tp)
    first = int(round(100 * cfg.min_recall)) + 1
    levels = np.linspace(0, 1, N_LEVELS)
    precision, confidence = np.zeros((C, T, N_LEVELS)), np.zeros((C, T, N_LEVELS))
    err_curves, aps, tp_table = np.ones((C, 5, N_LEVELS)), np.zeros((C, T)), np.ones((C, 5))
    mri = np.zeros(C, np.int32)
    for c in range(C):
        o = order[cls_off[c]:cls_off[c + 1]]
        sc = scores[o].astype(np.float64)
        for t in range(T):
            flag = match[t, o] >= 0
            M = int(flag.sum())
            if npos[c] <= 0 or M == 0:
                continue  # the empty curve
            tp = np.cumsum(flag.astype(np.int64))
            prec = tp.astype(np.float64) / np.arange(1, o.size + 1).astype(np.float64)
            rec = tp.astype(np.float64) / float(npos[c])
            precision[c, t] = interp(levels, rec, prec, right=0.0)
            confidence[c, t] = interp(levels, rec, sc, right=0.0)
            aps[c, t] = (_seq_sum(np.maximum(precision[c, t, first:] - cfg.min_precision, 0.0)) / float(N_LEVELS - first)) / \
                (1.0 - cfg.min_precision)
            if t != tp_idx:
                continue
            ms = sc[flag]
            e = errors[o[flag]]
            for q in range(5):
                if q == 4:
                    cm = np.ones(M) if attr_empty[c] else np.zeros(M)
                else:
                    cm = np.cumsum(e[:, q]) / np.arange(1, M + 1).astype(np.float64)
                err_curves[c, q] = interp(confidence[c, t][::-1], ms[::-1], cm[::-1])[::-1]
            nz = np.flatnonzero(confidence[c, t])
            last = int(nz[-1]) if nz.size else 0
            mri[c] = last
            if last >= first:
                for q in range(5):
                    tp_table[c, q] = _seq_sum(err_curves[c, q, first:last + 1]) / float(last - first + 1)
    return dict(precision=precision, confidence=confidence, err_curves=err_curves, aps=aps, tp_table=tp_table, max_recall_ind=mri)


def summarize(tables, cfg):
    """The devkit's DetectionMetrics.serialize() keys from the [C, T] APs and [C, 5] TP errors (host, float64)."""
    names = list(cfg.class_names)
    aps = np.asarray(tables["aps"], np.float64)
    tpt = np.array(tables["tp_table"], np.float64)
    for c, n in enumerate(names):
        if n == "traffic_cone":
            tpt[c, [4, 3, 2]] = np.nan
        elif n == "barrier":
            tpt[c, [4, 3]] = np.nan
    label_aps = {n: {th: float(aps[c, t]) for t, th in enumerate(cfg.dist_ths)} for c, n in enumerate(names)}
    mean_dist_aps = {n: _seq_sum(aps[c]) / float(aps.shape[1]) for c, n in enumerate(names)}
    mean_ap = _seq_sum(mean_dist_aps.values()) / float(len(names))
    label_tp = {n: {k: float(tpt[c, q]) for q, k in enumerate(TP_METRICS)} for c, n in enumerate(names)}
    tp_errors, tp_scores = {}, {}
    for q, k in enumerate(TP_METRICS):
        col = tpt[:, q][~np.isnan(tpt[:, q])]
        tp_errors[k] = _seq_sum(col) / float(col.size) if col.size else float("nan")
        tp_scores[k] = 1.0 - min(1.0, tp_errors[k]) if col.size else 0.0
    total = float(cfg.mean_ap_weight) * mean_ap + _seq_sum(tp_scores.values())
    nd_score = total / float(cfg.mean_ap_weight + len(tp_scores))
    return dict(label_aps=label_aps, mean_dist_aps=mean_dist_aps, mean_ap=mean_ap, label_tp_errors=label_tp, tp_errors=tp_errors,
                tp_scores=tp_scores, nd_score=nd_score, cfg=cfg.serialize())


def numpy_detection_eval(preds, gts, cfg, classes):
    """The specification (module docstring), plain numpy on the host."""
    preds = [_unpack_pred(p) for p in preds]
    _check_counts(preds, gts, cfg)
    _, period, attr_empty = _class_tables(cfg, classes)
    P, scores, p_cls, p_off = pack_preds_numpy(preds, cfg, classes)
    G, g_cls, g_off = pack_gt(gts, cfg, classes)
    C = len(cfg.class_names)
    match, errors = numpy_match(P, scores, p_cls, p_off, G, g_cls, g_off, cfg, period, attr_empty)
    order, cls_off = global_order(scores, p_cls, C)
    npos = np.bincount(g_cls[g_cls >= 0], minlength=C).astype(np.int32)
    tables = numpy_curves(scores, order, cls_off, match, errors, npos, cfg, attr_empty)
    out = summarize(tables, cfg)
    out.update(tables, match=match, pred_errors=errors)
    return out


# ------------------------------------------------------------------------------------------------------------ the kernels
def max_preds():
    """The most predictions per sample the kernels take (bfhip_detection_eval_max_preds)."""
    return int(_lib.load().bfhip_detection_eval_max_preds())


def max_gt():
    """The most GT boxes per (sample, class) the kernels take (bfhip_detection_eval_max_gt)."""
    return int(_lib.load().bfhip_detection_eval_max_gt())


def kernel_supported(preds, g_cls, g_off, cfg, n_dataset_classes=1):
    """True when csrc/detection_eval.hip takes the call: every sample's boxes float32 [n, 7 or 9], scores float32 and integer
    labels as tensors on ONE device, at least one prediction, at most max_preds() per sample and max_gt() GT per (sample, class),
    class and threshold counts within the library's."""
    lib = _lib.load()
    C, T = len(cfg.class_names), len(cfg.dist_ths)
    if not (1 <= C <= lib.bfhip_detection_eval_max_classes() and 1 <= T <= lib.bfhip_detection_eval_max_thresholds()):
        return False
    if n_dataset_classes < 1 or not preds:
        return False
    dev, total = None, 0
    for b, s, l in preds:
        b = getattr(b, "tensor", b)
        if not (torch.is_tensor(b) and torch.is_tensor(s) and torch.is_tensor(l) and b.is_cuda and s.is_cuda and l.is_cuda):
            return False
        if dev is None:
            dev = b.device
        if b.device != dev or s.device != dev or l.device != dev or b.dtype != torch.float32 or s.dtype != torch.float32 or \
                l.dtype.is_floating_point or l.dtype == torch.bool:
            return False
        if b.dim() != 2 or b.shape[1] not in (7, 9) or s.dim() != 1 or l.dim() != 1 or b.shape[0] != s.shape[0] or \
                l.shape[0] != s.shape[0] or s.shape[0] > max_preds():
            return False
        total += int(s.shape[0])
    if total == 0 or total >= (1 << 31) or g_cls.shape[0] >= (1 << 31):
        return False
    if g_cls.size:
        sample = np.repeat(np.arange(len(g_off) - 1), np.diff(g_off))
        ok = g_cls >= 0
        if ok.any() and np.bincount(sample[ok].astype(np.int64) * C + g_cls[ok]).max() > max_gt():
            return False
    return True


def _mask(bits):
    return int(sum(1 << i for i, b in enumerate(bits) if b))


def kernel_detection_eval(preds, G, g_cls, g_off, cfg, classes):
    """The device path -> the raw tables; `match` and `pred_errors` stay on the device.  One host synchronisation, at the end."""
    lut, period, attr_empty = _class_tables(cfg, classes)
    C, T, S = len(cfg.class_names), len(cfg.dist_ths), len(preds)
    tp_idx = list(cfg.dist_ths).index(cfg.dist_th_tp)
    first = int(round(100 * cfg.min_recall)) + 1
    dev = getattr(preds[0][0], "tensor", preds[0][0]).device
    boxes = [getattr(b, "tensor", b) for b, _, _ in preds]
    if all(b.shape[1] == 9 for b in boxes):
        P = torch.cat(boxes, 0).contiguous()
    else:
        P = torch.cat([b if b.shape[1] == 9 else torch.nn.functional.pad(b, (0, 2)) for b in boxes], 0).contiguous()
    scores = torch.cat([s for _, s, _ in preds], 0).contiguous()
    labels = torch.cat([l for _, _, l in preds], 0).long()
    Np = int(scores.shape[0])
    p_off = np.concatenate([[0], np.cumsum([int(s.shape[0]) for _, s, _ in preds])]).astype(np.int32)
    npos = np.bincount(g_cls[g_cls >= 0], minlength=C).astype(np.int32)

    # one pinned upload of every host table: int32 (lut, p_off, g_off, g_cls, npos), float32 G, float64 levels
    ints = np.concatenate([lut, p_off, g_off, g_cls, npos]).astype(np.int32)
    n_i, n_g = ints.size + (ints.size & 1), G.size + (G.size & 1)  # float64 part 8-byte aligned
    host = torch.empty((n_i + n_g) * 4 + N_LEVELS * 8, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    hv[:ints.size * 4] = ints.view(np.uint8)
    hv[n_i * 4:n_i * 4 + G.size * 4] = G.reshape(-1).view(np.uint8)
    hv[(n_i + n_g) * 4:] = np.linspace(0, 1, N_LEVELS).view(np.uint8)
    table = torch.empty(host.shape[0], dtype=torch.uint8, device=dev)
    table.copy_(host, non_blocking=True)
    ti = table[:ints.size * 4].view(torch.int32)
    L = lut.size
    d_lut, d_poff, d_goff = ti[:L], ti[L:L + S + 1], ti[L + S + 1:L + 2 * S + 2]
    d_gcls, d_npos = ti[L + 2 * S + 2:L + 2 * S + 2 + g_cls.size], ti[ints.size - C:]
    d_G = table[n_i * 4:n_i * 4 + G.size * 4].view(torch.float32)
    d_levels = table[(n_i + n_g) * 4:].view(torch.float64)

    bad_label = (labels < 0) | (labels >= L)
    p_cls = d_lut[labels.clamp(0, L - 1)].masked_fill(bad_label, -1).contiguous()
    flags = torch.stack([torch.isfinite(P).all() & torch.isfinite(scores).all(), ~bad_label.any()])  # read with the tables

    match = torch.full((T, Np), -1, dtype=torch.int32, device=dev)
    errors = torch.full((Np, 5), float("nan"), dtype=torch.float64, device=dev)
    ths = (np.ctypeslib.as_ctypes(np.asarray(cfg.dist_ths, np.float64)))
    half_mask = _mask(period == np.pi)
    attr_mask = _mask(attr_empty)
    stream = _lib.stream_of(scores)
    with torch.cuda.device(dev):
        _lib.call("bfhip_detection_match", P.data_ptr(), scores.data_ptr(), p_cls.data_ptr(), d_poff.data_ptr(), Np,
                  d_G.data_ptr() if G.size else None, d_gcls.data_ptr() if g_cls.size else None, d_goff.data_ptr(),
                  int(g_cls.size), S, C, ths, T, tp_idx, half_mask, attr_mask, match.data_ptr(), errors.data_ptr(), stream)
        # the global order: stable sorts of the flipped arrays, so that equal scores keep the HIGHER flat index first
        o1 = torch.argsort(scores.flip(0), descending=True, stable=True)
        flat = (Np - 1) - o1
        key = torch.where(p_cls < 0, torch.full_like(p_cls, C), p_cls)[flat]
        o2 = torch.argsort(key, stable=True)
        order = flat[o2].to(torch.int32).contiguous()
        cls_off = torch.searchsorted(key[o2].contiguous(), torch.arange(C + 1, device=dev, dtype=key.dtype)).to(torch.int32)
        n_out = 2 * C * T * N_LEVELS + C * 5 * N_LEVELS + C * T + C * 5
        out = torch.empty(n_out, dtype=torch.float64, device=dev)
        mri = torch.empty(C, dtype=torch.int32, device=dev)
        a = C * T * N_LEVELS
        b = a * 2 + C * 5 * N_LEVELS
        o_prec, o_conf, o_err, o_ap, o_tp = out[:a], out[a:2 * a], out[2 * a:b], out[b:b + C * T], out[b + C * T:]
        nbytes = _lib.call_size("bfhip_detection_curves_workspace_bytes", Np, T)
        work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.call("bfhip_detection_curves", scores.data_ptr(), order.data_ptr(), cls_off.data_ptr(), match.data_ptr(),
                  errors.data_ptr(), Np, C, T, tp_idx, d_npos.data_ptr(), d_levels.data_ptr(), float(cfg.min_precision), first,
                  attr_mask, o_prec.data_ptr(), o_conf.data_ptr(), o_err.data_ptr(), o_ap.data_ptr(), o_tp.data_ptr(),
                  mri.data_ptr(), work.data_ptr(), nbytes, stream)
    h_flags = flags.cpu()  # the first host read: it waits for everything above
    if not bool(h_flags[0]):
        raise ValueError("detection_eval: a non-finite score or box value")
    if not bool(h_flags[1]):
        raise ValueError("detection_eval: a prediction label outside [0, %d)" % L)
    h = out.cpu().numpy()
    return dict(precision=h[:a].reshape(C, T, N_LEVELS), confidence=h[a:2 * a].reshape(C, T, N_LEVELS),
                err_curves=h[2 * a:b].reshape(C, 5, N_LEVELS), aps=h[b:b + C * T].reshape(C, T), tp_table=h[b + C * T:].reshape(C, 5),
                max_recall_ind=mri.cpu().numpy(), match=match, pred_errors=errors)


def detection_eval(preds, gts, cfg=None, classes=None):
    """numpy_detection_eval's results through the kernels when they take the call (then `match` and `pred_errors` are device
    tensors, otherwise arrays)."""
    cfg = cfg if cfg is not None else config_factory()
    classes = list(classes if classes is not None else cfg.class_names)
    preds = [_unpack_pred(p) for p in preds]
    _check_counts(preds, gts, cfg)
    G, g_cls, g_off = pack_gt(gts, cfg, classes)
    if not (ENABLED and kernel_supported(preds, g_cls, g_off, cfg, len(classes))):
        PATHS["torch"] += 1
        return numpy_detection_eval(preds, gts, cfg, classes)
    PATHS["kernel"] += 1
    tables = kernel_detection_eval(preds, G, g_cls, g_off, cfg, classes)
    out = summarize(tables, cfg)
    out.update(tables)
    return out


# ------------------------------------------------------------------------------------------------------------- the metric
def _fmt(v):
    return "nan" if isinstance(v, float) and math.isnan(v) else "%.2f" % v


def format_nuscenes_metrics(metrics, class_names, version="default"):
    """(table string, details dict): the reference's per-class table (functional/nuscenes_utils/utils.py:229-266: mAP, AP@<t>m,
    error@<metric> without attr_err, two decimals) as a pipe table, and its `details` keys: the tp_errors keys, mAP_<class>, mAP,
    NDS."""
    rows, columns = [], None
    for name in class_names:
        aps, errs = metrics["label_aps"][name], metrics["label_tp_errors"][name]
        row = {"mAP": sum(aps.values()) * 100 / len(aps)}
        row.update({"AP@%sm" % k: v * 100 for k, v in aps.items()})
        row.update({"error@%s" % k: v for k, v in errs.items() if k != "attr_err"})
        columns = columns or list(row)
        rows.append([name] + [_fmt(float(row[k])) for k in columns])
    head = ["class_name"] + (columns or [])
    width = [max(len(r[i]) for r in [head] + rows) for i in range(len(head))]
    line = lambda r: "| " + " | ".join([r[0].ljust(width[0])] + [x.rjust(w) for x, w in zip(r[1:], width[1:])]) + " |"  # noqa: E731
    sep = "|" + "|".join([":" + "-" * (width[0] + 1)] + ["-" * (w + 1) + ":" for w in width[1:]]) + "|"
    result = "----------------nuScenes %s results-----------------\n" % version + "\n".join([line(head), sep] + [line(r) for r in rows])
    details = dict(metrics["tp_errors"])
    details.update({"mAP_%s" % k: v for k, v in metrics["mean_dist_aps"].items()})
    details.update(mAP=metrics["mean_ap"], NDS=metrics["nd_score"])
    return result, details


@METRICS.register_module()
class NuScenesCustomMetric:
    """The reference's evaluator of its custom-data configs (metrics/nuscenes_custom_metric.py:184-807), same constructor
    keywords; `data_list=` passes the infos directly, `ann_file` may be a .pkl or .json holding a `data_list`.  process() keeps the
    predictions on their device; compute_metrics() runs detection_eval on them."""

    CLASSES = ("car", "truck", "bus", "bicycle", "pedestrian")
    DefaultAttribute = DEFAULT_ATTRIBUTE
    ErrNameMapping = ERR_NAME_MAPPING
    default_prefix = "NuScenes metric"

    def __init__(self, data_root=None, ann_file=None, metric="bbox", modality=None, prefix=None, format_only=False,
                 jsonfile_prefix=None, eval_version="detection_cvpr_2019", collect_device="cpu", backend_args=None, data_list=None):
        self.data_root, self.ann_file, self.prefix, self.collect_device = data_root, ann_file, prefix, collect_device
        self.modality = modality if modality is not None else dict(use_camera=False, use_lidar=True)
        self.format_only = format_only
        if format_only:
            assert jsonfile_prefix is not None, "jsonfile_prefix must be not None when format_only is True"
        self.jsonfile_prefix, self.backend_args = jsonfile_prefix, backend_args
        self.metrics = metric if isinstance(metric, list) else [metric]
        self.eval_version = eval_version
        self.eval_detection_configs = config_factory(eval_version)
        self.dataset_meta = dict(classes=self.CLASSES, version="custom")
        self.data_infos = data_list
        self.results = []

    def load_infos(self):
        if self.data_infos is None:
            path = self.ann_file if self.data_root is None or os.path.isabs(self.ann_file) or os.path.exists(self.ann_file) \
                else os.path.join(self.data_root, self.ann_file)
            if path.endswith(".json"):
                with open(path) as f:
                    self.data_infos = json.load(f)["data_list"]
            else:
                with open(path, "rb") as f:
                    self.data_infos = pickle.load(f)["data_list"]
        return self.data_infos

    def process(self, data_batch, data_samples):
        """Collects one batch: the reference's {'pred_instances_3d': {bboxes_3d, scores_3d, labels_3d}, 'sample_idx'} or predict()'s
        {bboxes_3d, scores_3d, labels_3d} with 'sample_idx'.  The tensors stay where they are."""
        for i, sample in enumerate(data_samples):
            pred = sample["pred_instances_3d"] if "pred_instances_3d" in sample else sample
            idx = sample.get("sample_idx")
            if idx is None and isinstance(data_batch, dict) and "sample_idx" in data_batch:
                idx = data_batch["sample_idx"][i]
            if idx is None:
                raise KeyError("sample_idx")
            boxes = getattr(pred["bboxes_3d"], "tensor", pred["bboxes_3d"])
            self.results.append(dict(pred_instances_3d=dict(bboxes_3d=boxes, scores_3d=pred["scores_3d"], labels_3d=pred["labels_3d"]),
                                     sample_idx=int(idx)))

    def _tokens(self, infos):
        return [info.get("token", i) for i, info in enumerate(infos)]

    def _gather(self, results, infos):
        """(preds, gts) in the infos' order; the reference's assertion on the sample sets."""
        by_idx = {}
        for r in results:
            by_idx[int(r["sample_idx"])] = r["pred_instances_3d"]  # a repeated sample: the last one, as the reference's dict
        tokens = self._tokens(infos)
        pred_tokens = {tokens[i] if 0 <= i < len(tokens) else ("?", i) for i in by_idx}
        assert pred_tokens == set(tokens), "Samples in split doesn't match samples in predictions."
        token_idx = {}
        for i, t in enumerate(tokens):
            token_idx[t] = i
        keep = sorted(token_idx.values())  # infos sharing a token: the last, as the reference's dict
        preds = [(by_idx[i]["bboxes_3d"], by_idx[i]["scores_3d"], by_idx[i]["labels_3d"]) for i in keep]
        gts = []
        for i in keep:
            inst = infos[i].get("instances", [])
            gts.append((np.array([x["bbox_3d"] for x in inst], np.float64).reshape(len(inst), -1),
                        np.array([x["bbox_label_3d"] for x in inst], np.int64)))
        return preds, gts

    def format_results(self, results, classes, jsonfile_prefix):
        """Writes <jsonfile_prefix>/pred_instances_3d/results_nusc.json with the reference's keys (_format_lidar_bbox); the
        rotation is (cos(yaw / 2), 0, 0, sin(yaw / 2)), the size (dy, dx, dz)."""
        infos = self.load_infos()
        tokens = self._tokens(infos)
        annos = {}
        for r in results:
            p = r["pred_instances_3d"]
            b, s, l = pred_lidar_boxes(_np(p["bboxes_3d"])), _np(p["scores_3d"]), _np(p["labels_3d"])
            token = tokens[int(r["sample_idx"])]
            rows = []
            for k in range(b.shape[0]):
                name = classes[int(l[k])]
                yaw = float(b[k, 6])
                rows.append(dict(sample_token=token, translation=[float(v) for v in b[k, :3]],
                                 size=[float(b[k, 4]), float(b[k, 3]), float(b[k, 5])],
                                 rotation=[math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)], velocity=[float(b[k, 7]), float(b[k, 8])],
                                 detection_name=name, detection_score=float(s[k]), attribute_name=self.DefaultAttribute[name]))
            annos[token] = rows
        out_dir = os.path.join(jsonfile_prefix, "pred_instances_3d")
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "results_nusc.json")
        with open(path, "w") as f:
            json.dump(dict(meta=self.modality, results=annos), f)
        return path

    def compute_metrics(self, results):
        """dict(result=<the table>) as the reference's _evaluate_single, plus the `details` entries and 'metrics', the full
        dict of detection_eval.  format_only: writes the JSON and returns {}."""
        classes = list(self.dataset_meta["classes"])
        if self.format_only:
            self.format_results(results, classes, self.jsonfile_prefix)
            return {}
        infos = self.load_infos()
        preds, gts = self._gather(results, infos)
        metrics = detection_eval(preds, gts, self.eval_detection_configs, classes)
        table, details = format_nuscenes_metrics(metrics, sorted(set(self.CLASSES), key=self.CLASSES.index))
        out = dict(result=table)
        out.update(details)
        out["metrics"] = metrics
        return out

    def evaluate(self, size=None):
        """compute_metrics on what process() collected; the collection is emptied, as mmengine's BaseMetric does."""
        out = self.compute_metrics(self.results)
        self.results = []
        return out
