"""GPU: csrc/detection_eval.hip (bfhip_detection_match / bfhip_detection_curves) against its specification
(evaluation.numpy_detection_eval): match, the per-prediction errors, precision, confidence, the APs and max_recall_ind bit for
bit, the error curves and TP scalars within the re-ordered sums' bound; the fallbacks, the argument checks and the metric class
on device tensors."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import detection_eval_cases as dc
from bevfusion_amd import _lib
from bevfusion_amd import evaluation as ev
from bevfusion_amd.registry import METRICS

pytestmark = pytest.mark.gpu
CFG = ev.config_factory()
U = 2.0 ** -53

# name -> (classes, [(seed, samples, GT per (sample, class), predictions per sample, columns)]): the parts are concatenated
CASES = {
    "no_gt": (dc.CLASSES5, [(1, 1, 0, 1, 9)]),
    "one_wave": (dc.CLASSES5, [(2, 1, 64, 64, 7)]),
    "mixed10": (dc.CLASSES10, [(3, 1, 1, 0, 9), (4, 1, 63, 64, 9), (5, 1, 64, 500, 9)]),
    "words5": (dc.CLASSES5, [(6, 1, 65, 500, 9), (7, 1, 130, 64, 9), (8, 1, 130, 500, 9)]),
    "many10": (dc.CLASSES10, [(9, 70, 1, 64, 9)]),
    "three5": (dc.CLASSES5, [(10, 3, 5, 64, 7)]),
}


def build(name):
    classes, parts = CASES[name]
    preds, gts = [], []
    for seed, s, g, p, dim in parts:
        a, b = dc.random_case(seed, s, g, p, classes, pred_dim=dim)
        preds += a
        gts += b
    return classes, preds, gts


def to_dev(preds, dev):
    return [(torch.from_numpy(b).to(dev), torch.from_numpy(s).to(dev), torch.from_numpy(l).to(dev)) for b, s, l in preds]


@pytest.fixture(scope="module")
def reference():
    """Every case and its specification result, computed once."""
    out = {}
    for name in CASES:
        classes, preds, gts = build(name)
        out[name] = (classes, preds, gts, ev.numpy_detection_eval(preds, gts, CFG, classes))
    return out


def matched_count(res, preds, classes):
    """The largest number of matched predictions of one class at dist_th_tp: the terms of the longest cumulative sum."""
    tp_idx = list(CFG.dist_ths).index(CFG.dist_th_tp)
    p_cls = ev.pack_preds_numpy(preds, CFG, classes)[2]
    hit = np.asarray(res["match"])[tp_idx] >= 0
    return int(np.bincount(p_cls[hit & (p_cls >= 0)], minlength=1).max())


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def assert_same(got, want, n):
    for k in ("match", "pred_errors", "precision", "confidence", "aps", "max_recall_ind"):
        g, w = host(got[k]), host(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, k
        assert np.array_equal(dc.bits(g), dc.bits(w)), k
    rtol = 2 * max(n - 1, 0) * U
    for k in ("err_curves", "tp_table"):
        np.testing.assert_allclose(host(got[k]), host(want[k]), rtol=rtol, atol=0, err_msg=k)
    assert got["mean_ap"] == want["mean_ap"]
    # nd_score = (5 mean_ap + sum of five 1 - min(1, e)) / 10 with mean_ap exact: each clipped e <= 1 is off by at most rtol
    # ABSOLUTE (the subtraction from 1 loses the relative bound), so the score by at most rtol / 2 plus the few roundings after
    np.testing.assert_allclose(got["nd_score"], want["nd_score"], rtol=0, atol=rtol / 2 + 4 * U)


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_specification(dev, reference, name):
    classes, preds, gts, want = reference[name]
    before = dict(ev.PATHS)
    got = ev.detection_eval(to_dev(preds, dev), gts, CFG, classes)
    assert ev.PATHS["kernel"] == before["kernel"] + 1 and ev.PATHS["torch"] == before["torch"]
    assert got["match"].is_cuda and got["pred_errors"].is_cuda
    n = max(matched_count(r[3], r[1], r[0]) for r in reference.values())
    print("%s: %d predictions, %d matched of one class at dist_th_tp, largest matched count %d, rtol %.3g" %
          (name, host(got["match"]).shape[1], matched_count(want, preds, classes), n, 2 * (n - 1) * U))
    assert_same(got, want, n)


def test_inputs_are_not_degenerate(reference):
    ties = taken = matched = unmatched = 0
    for name, (classes, preds, gts, want) in reference.items():
        a, b, c, d = dc.input_properties(preds, gts, want, CFG)
        ties, taken, matched, unmatched = ties + a, taken + b, matched + c, unmatched + d
    assert ties > 100 and taken > 20 and matched > 500 and unmatched > 500, (ties, taken, matched, unmatched)
    on_threshold = 0
    for classes, preds, gts, want in reference.values():
        e = host(want["pred_errors"])[:, 0]
        on_threshold += int(np.isin(e, [0.5, 1.0]).sum())  # exactly a smaller threshold: unmatched there, by the strict <
    assert on_threshold > 0


def test_worked_case_through_the_kernel(dev):
    for third in (False, True):
        preds, gts = dc.worked_case(third)
        want = ev.numpy_detection_eval(preds, gts, CFG, dc.CLASSES5)
        got = ev.detection_eval(to_dev(preds, dev), gts, CFG, dc.CLASSES5)
        assert_same(got, want, 2)
        assert abs(got["label_aps"]["car"][2.0] - (0.4524691358024691 if third else 0.7376543209876539)) < 1e-9


def test_two_calls_same_bytes(dev, reference):
    classes, preds, gts, _ = reference["words5"]
    d = to_dev(preds, dev)
    a, b = ev.detection_eval(d, gts, CFG, classes), ev.detection_eval(d, gts, CFG, classes)
    for k in ("match", "pred_errors", "precision", "confidence", "err_curves", "aps", "tp_table", "max_recall_ind"):
        assert np.array_equal(dc.bits(host(a[k])), dc.bits(host(b[k]))), k


_CHILD = """
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import detection_eval_cases as dc
from bevfusion_amd import evaluation as ev
cfg = ev.config_factory()
preds, gts = dc.random_case(10, 3, 5, 64, dc.CLASSES5, pred_dim=7)
dev = torch.device("cuda:0")
r = ev.detection_eval([tuple(torch.from_numpy(a).to(dev) for a in p) for p in preds], gts, cfg, dc.CLASSES5)
assert ev.PATHS == {"kernel": 0, "torch": 1} and not ev.ENABLED, ev.PATHS
np.savez(sys.argv[1], **{k: np.asarray(r[k]) for k in ("match", "pred_errors", "precision", "confidence", "err_curves", "aps",
                                                       "tp_table", "max_recall_ind")})
"""


def test_fallbacks(dev, reference, tmp_path):
    # GT above the cap per (sample, class)
    cap = ev.max_gt()
    assert cap >= 1024 and ev.max_preds() >= 500
    rs = np.random.RandomState(0)
    g = np.zeros((cap + 1, 7))
    g[:, :2] = rs.randint(-100, 101, (cap + 1, 2)) * 0.5
    g[:, 3:6] = 1.0
    gts = [(g, np.zeros(cap + 1, np.int64))]
    p = np.zeros((40, 9), np.float32)
    p[:, :2] = g[rs.randint(0, cap + 1, 40), :2] + 0.25
    p[:, 3:6] = 1.0
    preds = [(p, dc.SCORES[rs.randint(0, 7, 40)], np.zeros(40, np.int64))]
    before = dict(ev.PATHS)
    got = ev.detection_eval(to_dev(preds, dev), gts, CFG, dc.CLASSES5)
    assert ev.PATHS["torch"] == before["torch"] + 1 and ev.PATHS["kernel"] == before["kernel"]
    assert_same(got, ev.numpy_detection_eval(preds, gts, CFG, dc.CLASSES5), 0)
    # ... and exactly at the cap the kernel takes it
    gts_cap = [(g[:cap], np.zeros(cap, np.int64))]
    got = ev.detection_eval(to_dev(preds, dev), gts_cap, CFG, dc.CLASSES5)
    assert ev.PATHS["kernel"] == before["kernel"] + 1
    assert_same(got, ev.numpy_detection_eval(preds, gts_cap, CFG, dc.CLASSES5), 40)
    # CPU tensors
    classes, preds, gts, want = reference["three5"]
    before = dict(ev.PATHS)
    got = ev.detection_eval([tuple(torch.from_numpy(a) for a in q) for q in preds], gts, CFG, classes)
    assert ev.PATHS["torch"] == before["torch"] + 1
    assert_same(got, want, 0)
    # BFHIP_DETECTION_EVAL=0 in a fresh process
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=root, tests=os.path.join(root, "tests")), str(tmp_path / "out.npz")],
                       env=dict(os.environ, BFHIP_DETECTION_EVAL="0"), capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    child = np.load(str(tmp_path / "out.npz"))
    assert_same(dict(child, mean_ap=want["mean_ap"], nd_score=want["nd_score"]), want, 0)


def test_invalid_inputs_raise_on_the_device(dev):
    preds, gts = dc.worked_case()
    bad = [(preds[0][0], np.array([0.9, np.nan, 0.7], np.float32), preds[0][2])]
    with pytest.raises(ValueError, match="non-finite"):
        ev.detection_eval(to_dev(bad, dev), gts, CFG, dc.CLASSES5)
    bad = [(preds[0][0], preds[0][1], np.array([0, 5, 0]))]
    with pytest.raises(ValueError, match="label"):
        ev.detection_eval(to_dev(bad, dev), gts, CFG, dc.CLASSES5)


def test_c_entries_reject_invalid_arguments(dev):
    lib = _lib.load()
    buf = torch.full((4096,), 7, dtype=torch.int32, device=dev)
    ptr = buf.data_ptr()
    ths = (ctypes.c_double * 4)(0.5, 1.0, 2.0, 4.0)
    stream = _lib.stream_of(buf)

    def match(**kw):
        a = dict(pred=ptr, score=ptr, pred_cls=ptr, pred_off=ptr, n_pred=4, gt=ptr, gt_cls=ptr, gt_off=ptr, n_gt=4, S=1, C=5,
                 ths=ths, T=4, tp=2, match=ptr, err=ptr)
        a.update(kw)
        return lib.bfhip_detection_match(a["pred"], a["score"], a["pred_cls"], a["pred_off"], a["n_pred"], a["gt"], a["gt_cls"],
                                         a["gt_off"], a["n_gt"], a["S"], a["C"], a["ths"], a["T"], a["tp"], 0, 0, a["match"],
                                         a["err"], stream)

    for kw in (dict(T=0), dict(T=9), dict(tp=4), dict(C=0), dict(C=65), dict(n_pred=-1), dict(pred=None), dict(match=None),
               dict(gt=None), dict(ths=None), dict(pred_off=None), dict(n_gt=1 << 31), dict(err=ptr + 4), dict(score=ptr + 2)):
        assert match(**kw) != 0, kw
        assert lib.bfhip_last_error().decode().startswith("detection_match"), kw

    def curves(**kw):
        a = dict(n_pred=4, C=5, T=4, tp=2, first=11, order=ptr, out=ptr, ws=ptr, ws_bytes=1 << 14)
        a.update(kw)
        return lib.bfhip_detection_curves(ptr, a["order"], ptr, ptr, ptr, a["n_pred"], a["C"], a["T"], a["tp"], ptr, ptr, 0.1,
                                          a["first"], 0, a["out"], ptr, ptr, ptr, ptr, ptr, a["ws"], a["ws_bytes"], stream)

    assert lib.bfhip_detection_curves_workspace_bytes(4, 4) <= 1 << 14
    assert lib.bfhip_detection_curves_workspace_bytes(-1, 4) == 0 and lib.bfhip_detection_curves_workspace_bytes(4, 9) == 0
    for kw in (dict(n_pred=0), dict(C=65), dict(T=0), dict(tp=-1), dict(first=101), dict(order=None), dict(out=None),
               dict(ws=ptr + 4), dict(ws_bytes=8), dict(ws=None)):
        assert curves(**kw) != 0, kw
        assert lib.bfhip_last_error().decode().startswith("detection_curves"), kw
    torch.cuda.synchronize()
    assert bool((buf == 7).all())  # nothing was launched: nothing was written


def test_metric_on_device_tensors(dev, reference):
    classes, preds, gts, _ = reference["three5"]
    preds, gts = preds + preds[:1], gts + gts[:1]
    infos = [dict(token="t%d" % i, instances=[dict(bbox_3d=list(map(float, b)), bbox_label_3d=int(l)) for b, l in zip(*gts[i])])
             for i in range(4)]
    metric = METRICS.build(dict(type="NuScenesCustomMetric", data_list=infos))
    d = to_dev(preds, dev)
    before = dict(ev.PATHS)
    for batch in ([2, 0], [3], [1]):  # several batches, out of order
        metric.process({}, [dict(bboxes_3d=d[i][0], scores_3d=d[i][1], labels_3d=d[i][2].int(), sample_idx=i) for i in batch])
    assert all(v.is_cuda for r in metric.results for v in r["pred_instances_3d"].values())
    out = metric.compute_metrics(metric.results)
    assert ev.PATHS["kernel"] == before["kernel"] + 1
    want = ev.numpy_detection_eval(preds, gts, CFG, list(metric.CLASSES))
    assert_same(out["metrics"], want, matched_count(want, preds, list(metric.CLASSES)))
    assert out["mAP"] == want["mean_ap"] and "car" in out["result"]
