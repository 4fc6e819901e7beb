#!/usr/bin/env python3
"""The nuScenes detection protocol on the device: evaluation.detection_eval (csrc/detection_eval.hip) against its specification,
evaluation.numpy_detection_eval, on one host core of the same machine.

Two synthetic validation sets, the predictions already on the device as predict() leaves them (one tensor triple per sample):

  nuscenes_val   6 019 samples x 200 predictions, 10 classes, about 30 GT boxes per sample
  custom_val     1 000 samples x 500 predictions, 5 classes, about 30 GT boxes per sample

Half of the predictions sit near a GT box of their class (offsets up to a few metres), the rest anywhere; scores are float32
sigmoid values with ties.  Per set one JSON entry:

  kernel   detection_eval(...): packing the GT on the host, concatenating the predictions on the device, one pinned upload, the
           match launch, two stable device sorts, the curves launch, the host read of the tables and the summary -- the call as
           NuScenesCustomMetric.compute_metrics makes it.  A host clock around one call; median of TIMED calls after WARMUP.
  host     numpy_detection_eval(...) on host copies of the same inputs (the copies are made before the clock starts), ONE thread.
           HOST_REPEATS calls, median.

The tables of the two are compared first: match, precision, confidence and the APs bit for bit, the error curves and TP errors
within the bound of a re-ordered sum.  A missing GPU is an error.  Usage: detection_eval_micro.py [OUT.json]   (default OUT: profiles/detection_eval_micro.json)"""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import evaluation as ev

CLASSES10 = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]
CLASSES5 = ["car", "truck", "bus", "bicycle", "pedestrian"]
SHAPES = (("nuscenes_val", 6019, 200, CLASSES10), ("custom_val", 1000, 500, CLASSES5))
GT_PER_SAMPLE = 30
WARMUP, TIMED, HOST_REPEATS = 2, 7, 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def draw(seed, samples, n_pred, classes):
    rs = np.random.RandomState(seed)
    C = len(classes)
    preds, gts = [], []
    for _ in range(samples):
        m = rs.poisson(GT_PER_SAMPLE)
        g = np.concatenate([rs.uniform(-50, 50, (m, 2)), rs.uniform(-2, 1, (m, 1)), rs.uniform(0.5, 8, (m, 3)), rs.uniform(-np.pi, np.pi, (m, 1))], 1)
        gl = rs.randint(0, C, m)
        p = np.concatenate([rs.uniform(-50, 50, (n_pred, 2)), rs.uniform(-3, 0, (n_pred, 1)), rs.uniform(0.5, 8, (n_pred, 3)),
                            rs.uniform(-np.pi, np.pi, (n_pred, 1)), rs.normal(size=(n_pred, 2))], 1).astype(np.float32)
        pl = rs.randint(0, C, n_pred)
        if m:
            near = rs.randint(0, m, n_pred // 2)
            p[:n_pred // 2, :2] = g[near, :2] + rs.normal(scale=1.0, size=(n_pred // 2, 2))
            pl[:n_pred // 2] = gl[near]
        score = (1.0 / (1.0 + np.exp(-rs.normal(-1.0, 1.5, n_pred)))).astype(np.float32)
        score[rs.rand(n_pred) < 0.05] = np.float32(0.1)  # ties
        preds.append((p, score, pl.astype(np.int64)))
        gts.append((g, gl.astype(np.int64)))
    return preds, gts


def measure(dev, name, samples, n_pred, classes):
    cfg = ev.config_factory()
    preds, gts = draw(samples, samples, n_pred, classes)
    on_dev = [tuple(torch.from_numpy(a).to(dev) for a in p) for p in preds]
    torch.cuda.synchronize()

    h_ms, want = [], None
    for _ in range(HOST_REPEATS):
        t0 = time.perf_counter()
        want = ev.numpy_detection_eval(preds, gts, cfg, classes)
        h_ms.append((time.perf_counter() - t0) * 1e3)
    print("# %s: host %.0f ms" % (name, median(h_ms)), flush=True)

    before = ev.PATHS["kernel"]
    got = ev.detection_eval(on_dev, gts, cfg, classes)
    assert ev.ENABLED and ev.PATHS["kernel"] == before + 1, "the kernel path did not take the call"
    assert np.array_equal(got["match"].cpu().numpy(), want["match"]), "match differs"
    for k in ("precision", "confidence", "aps"):
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64)), k
    tp_idx = list(cfg.dist_ths).index(cfg.dist_th_tp)
    matched = int((want["match"][tp_idx] >= 0).sum())
    rtol = 2.0 * max(matched - 1, 1) * 2.0 ** -53  # the bound of a re-ordered sum of that many non-negative terms
    np.testing.assert_allclose(got["tp_table"], want["tp_table"], rtol=rtol, atol=0)
    np.testing.assert_allclose(got["err_curves"], want["err_curves"], rtol=rtol, atol=0)

    k_ms = []
    for i in range(WARMUP + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.detection_eval(on_dev, gts, cfg, classes)
        torch.cuda.synchronize()
        if i >= WARMUP:
            k_ms.append((time.perf_counter() - t0) * 1e3)
    return dict(shape=name, samples=samples, predictions_per_sample=n_pred, classes=len(classes), gt_boxes=int(sum(len(l) for _, l in gts)),
                matched_at_dist_th_tp=matched, mean_ap=want["mean_ap"], nd_score=want["nd_score"],
                device=torch.cuda.get_device_name(0), warmup_calls=WARMUP, timed_calls=TIMED, launches_per_call="2 kernels + 2 sorts",
                kernel=dict(ms_per_call=round(median(k_ms), 3), min_max=[round(min(k_ms), 3), round(max(k_ms), 3)],
                            includes="GT packing on the host, device concatenation, 1 upload, match, 2 device sorts, curves, host "
                                     "read of the tables, summary"),
                host=dict(ms_per_call=round(median(h_ms), 1), min_max=[round(min(h_ms), 1), round(max(h_ms), 1)], threads=1,
                          calls=HOST_REPEATS),
                speedup=round(median(h_ms) / median(k_ms), 1), kernel_faster=max(k_ms) < min(h_ms), exact_tables_bit_equal=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("detection_eval_micro.py needs a GPU: nothing is measured without one")
    path = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "detection_eval_micro.json"))
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    lines = []
    for shape in SHAPES:
        lines.append(measure(dev, *shape))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
