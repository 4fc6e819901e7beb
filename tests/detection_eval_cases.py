"""Shared generators of the detection-evaluation tests (test_detection_eval_cpu.py, test_detection_eval_gpu.py)."""
import numpy as np

CLASSES10 = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
             "traffic_cone"]
CLASSES5 = ["car", "truck", "bus", "bicycle", "pedestrian"]
SCORES = np.array([0.9, 0.75, 0.5, 0.5, 0.3, 0.125, 0.05], np.float32)  # few values: ties occur


def box(x, y, z=0.0, dx=4.0, dy=2.0, dz=1.5, yaw=0.0, vx=None, vy=None):
    row = [x, y, z, dx, dy, dz, yaw]
    return row if vx is None else row + [vx, vy]


def worked_case(third_gt=False):
    """One sample, class car: GT centres (0, 0), (10, 0)[, (30, 30)]; predictions (0.2, 0) 0.9, (20, 0) 0.8, (10.6, 0) 0.7."""
    gt = [box(0, 0), box(10, 0)] + ([box(30, 30)] if third_gt else [])
    gts = [(np.array(gt, np.float64), np.zeros(len(gt), np.int64))]
    preds = [(np.array([box(0.2, 0, -0.75), box(20, 0, -0.75), box(10.6, 0, -0.75)], np.float32),
              np.array([0.9, 0.8, 0.7], np.float32), np.zeros(3, np.int64))]
    return preds, gts


def random_case(seed, n_samples, gt_per_class, n_pred, classes, pred_dim=9):
    """Seeded (preds, gts): per sample `gt_per_class` GT boxes of EVERY class (some duplicated) and `n_pred` predictions near
    them or far away; scores from SCORES; x, y on a 0.25 grid so that distances of exactly 0.5, 1, 2 and 4 occur and equidistant
    GT pairs exist."""
    rs = np.random.RandomState(seed)
    C = len(classes)
    preds, gts = [], []
    for _ in range(n_samples):
        m = gt_per_class * C
        g = np.zeros((m, 7))
        # few distinct sites per class: predictions compete for GT, and a taken nearest GT is common
        sites = max(1, min(gt_per_class, 12))
        g[:, 0] = rs.randint(-sites, sites + 1, m) * 3.0
        g[:, 1] = rs.randint(-2, 3, m) * 3.0
        g[:, 2] = rs.uniform(-1, 1, m)
        g[:, 3:6] = rs.uniform(0.5, 5.0, (m, 3))
        g[:, 6] = rs.uniform(-7.0, 7.0, m)
        gl = np.repeat(np.arange(C), gt_per_class)
        if m >= 2:
            dup = rs.randint(0, m, max(1, m // 8))
            g[dup] = g[np.clip(dup - 1, 0, m - 1)]  # the neighbour's box: mostly the same class
        if m:
            gl[rs.randint(0, m, 1 + m // 50)] = -1  # dropped labels
        gts.append((g, gl.astype(np.int64)))
        p = np.zeros((n_pred, pred_dim), np.float32)
        pl = rs.randint(0, C, n_pred)
        if n_pred:
            if m:
                near = rs.randint(0, m, n_pred)
                off = rs.choice([0.0, 0.25, 0.5, 1.0, 2.0, 4.0, -0.25, -0.5, -1.0, -2.0, 1.5, 7.0], (n_pred, 2))
                off[rs.rand(n_pred) < 0.5, 1] = 0.0
                p[:, :2] = g[near, :2] + off
                pl = np.where(rs.rand(n_pred) < 0.8, np.maximum(gl[near], 0), pl)
            else:
                p[:, :2] = rs.randint(-40, 41, (n_pred, 2)) * 0.25
            p[:, 2] = rs.uniform(-2, 0, n_pred)
            p[:, 3:6] = rs.uniform(0.5, 5.0, (n_pred, 3))
            p[:, 6] = rs.uniform(-7.0, 7.0, n_pred)
            if pred_dim == 9:
                p[:, 7:] = rs.choice([0.0, 0.5, -1.25, 3.0], (n_pred, 2))
        preds.append((p, SCORES[rs.randint(0, len(SCORES), n_pred)], pl.astype(np.int64)))
    return preds, gts


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def input_properties(preds, gts, res, cfg):
    """What a degenerate generator would lack: (score ties within a sample and class, predictions whose nearest GT of the class
    was already taken, matched predictions, unmatched predictions) as counts."""
    match = np.asarray(res["match"])
    tp_idx = list(cfg.dist_ths).index(cfg.dist_th_tp)
    ties = 0
    for (b, s, l) in preds:
        for c in np.unique(l):
            sc = s[l == c]
            ties += int(sc.size - np.unique(sc).size)
    taken = 0
    off_p = np.concatenate([[0], np.cumsum([len(s) for _, s, _ in preds])])
    # a prediction whose match is not the nearest GT of its class in the sample: the nearest was taken
    g_all, gl_all, g_off = [], [], [0]
    for g, gl in gts:
        keep = gl >= 0
        g_all.append(g[keep]), gl_all.append(gl[keep]), g_off.append(g_off[-1] + int(keep.sum()))
    g_all, gl_all = np.concatenate(g_all), np.concatenate(gl_all)
    for i, (b, s, l) in enumerate(preds):
        for k in range(len(s)):
            mt = match[tp_idx, off_p[i] + k]
            if mt < 0:
                continue
            cand = g_off[i] + np.flatnonzero(gl_all[g_off[i]:g_off[i + 1]] == gl_all[mt])
            d = np.hypot(g_all[cand, 0].astype(np.float32) - b[k, 0], g_all[cand, 1].astype(np.float32) - b[k, 1])
            taken += int(cand[np.argmin(d)] != mt)
    return ties, taken, int((match[tp_idx] >= 0).sum()), int((match[tp_idx] < 0).sum())
