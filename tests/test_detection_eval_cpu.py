"""CPU: the specification of the detection evaluation (bevfusion_amd/evaluation.py: numpy_detection_eval), the metric class around
it and its formatting.  No GPU, no kernel."""
import json
import math

import numpy as np
import pytest
import torch

import detection_eval_cases as dc
from bevfusion_amd import evaluation as ev
from bevfusion_amd.registry import METRICS

CFG = ev.config_factory()


def run(preds, gts, classes=dc.CLASSES5, cfg=CFG):
    return ev.numpy_detection_eval(preds, gts, cfg, classes)


def one_sample(gt_rows, gt_labels, pred_rows, scores, labels):
    return ([(np.array(pred_rows, np.float32), np.array(scores, np.float32), np.array(labels, np.int64))],
            [(np.array(gt_rows, np.float64), np.array(gt_labels, np.int64))])


def test_worked_case():
    r = run(*dc.worked_case())
    assert r["match"].tolist() == [[0, -1, -1], [0, -1, 1], [0, -1, 1], [0, -1, 1]]
    aps = r["label_aps"]["car"]
    for th in (1.0, 2.0, 4.0):
        assert abs(aps[th] - 0.7376543209876539) < 1e-9
    assert abs(aps[0.5] - 0.436213991769547) < 1e-9
    # (0.2 + 0.6) / 2 once both are matched, 0.2 before: float32(0.2), float32(10.6) - 10 widened
    assert abs(r["label_tp_errors"]["car"]["trans_err"] - 0.28500007496525) < 1e-9
    assert r["label_tp_errors"]["car"]["scale_err"] == 0.0 and r["label_tp_errors"]["car"]["orient_err"] == 0.0
    assert r["max_recall_ind"][0] == 100


def test_worked_case_with_an_unfound_gt():
    r = run(*dc.worked_case(third_gt=True))
    assert abs(r["label_aps"]["car"][2.0] - 0.4524691358024691) < 1e-9
    assert r["max_recall_ind"][0] == 66
    assert abs(r["label_tp_errors"]["car"]["trans_err"] - 0.28839293498145874) < 1e-9


def test_distance_on_the_threshold_is_no_match():
    p, g = one_sample([dc.box(0, 0)], [0], [dc.box(0, 2.0)], [0.5], [0])
    m = run(p, g)["match"]
    assert m[:, 0].tolist() == [-1, -1, -1, 0]  # d == 2.0 exactly: not at 2, matched at 4


def test_equidistant_gt_takes_the_lower_index():
    p, g = one_sample([dc.box(1, 0), dc.box(-1, 0)], [0, 0], [dc.box(0, 0)], [0.5], [0])
    assert run(p, g)["match"][2, 0] == 0
    p, g = one_sample([dc.box(-1, 0), dc.box(1, 0)], [0, 0], [dc.box(0, 0)], [0.5], [0])
    assert run(p, g)["match"][2, 0] == 0


def test_equal_scores_higher_flat_index_first():
    # both predictions reach only the one GT; the later row goes first and takes it
    p, g = one_sample([dc.box(0, 0)], [0], [dc.box(0.1, 0), dc.box(0.3, 0)], [0.5, 0.5], [0, 0])
    assert run(p, g)["match"][2].tolist() == [-1, 0]
    # across samples too: the flat index counts samples in evaluation order
    preds = [(np.array([dc.box(0.1, 0)], np.float32), np.array([0.5], np.float32), np.zeros(1, np.int64))] * 2
    gts = [(np.array([dc.box(0, 0)]), np.zeros(1, np.int64)), (np.zeros((0, 7)), np.zeros(0, np.int64))]
    r = run(preds, gts)
    # order: flat 1 (FP) then flat 0 (TP): precision at full recall is 1/2
    assert r["match"][2].tolist() == [0, -1] and r["precision"][0, 2, 100] == 0.5


def test_taken_gt_gives_the_next():
    p, g = one_sample([dc.box(0, 0), dc.box(1.5, 0)], [0, 0], [dc.box(0.1, 0), dc.box(0.2, 0)], [0.9, 0.8], [0, 0])
    assert run(p, g)["match"][2].tolist() == [0, 1]
    assert run(p, g)["match"][1].tolist() == [0, -1]  # 1.3 from the free one: no match at 1.0


def test_no_match_across_samples_or_classes():
    preds = [(np.array([dc.box(0, 0)], np.float32), np.array([0.5], np.float32), np.array([1]))] + \
        [(np.array([dc.box(0, 0)], np.float32), np.array([0.5], np.float32), np.array([0]))]
    gts = [(np.array([dc.box(0, 0)]), np.array([0])), (np.zeros((0, 7)), np.zeros(0, np.int64))]
    assert (run(preds, gts)["match"] == -1).all()


def test_barrier_period_and_nan_entries():
    classes = ["car", "barrier", "traffic_cone"]
    rows = [dc.box(0, 0, yaw=0.0), dc.box(10, 0, yaw=0.0), dc.box(20, 0, yaw=0.0)]
    prow = [dc.box(0, 0, -0.75, yaw=3.0), dc.box(10, 0, -0.75, yaw=3.0), dc.box(20, 0, -0.75, yaw=3.0)]
    p, g = one_sample(rows, [0, 1, 2], prow, [0.9, 0.9, 0.9], [0, 1, 2])
    r = run(p, g, classes)
    e = r["pred_errors"]
    assert abs(e[0, 2] - float(np.float32(3.0))) < 1e-12            # period 2 pi
    assert abs(e[1, 2] - (math.pi - 3.0)) < 1e-12                    # period pi
    assert e[0, 4] == 0.0 and math.isnan(e[1, 4]) and math.isnan(e[2, 4])
    tp = r["label_tp_errors"]
    assert all(math.isnan(tp["traffic_cone"][k]) for k in ("attr_err", "vel_err", "orient_err"))
    assert all(math.isnan(tp["barrier"][k]) for k in ("attr_err", "vel_err")) and not math.isnan(tp["barrier"]["orient_err"])
    assert not any(math.isnan(v) for v in tp["car"].values())


def test_class_without_gt_and_nd_score():
    r = run(*dc.worked_case())
    assert all(v == 0.0 for v in r["label_aps"]["truck"].values())
    assert all(v == 1.0 for v in r["label_tp_errors"]["truck"].values())
    assert (r["err_curves"][1] == 1.0).all() and (r["precision"][1] == 0.0).all()
    names = CFG.class_names
    mean_ap = sum(sum(r["label_aps"][n].values()) / 4 for n in names) / len(names)
    assert abs(r["mean_ap"] - mean_ap) < 1e-15
    errs = {k: np.nanmean([r["label_tp_errors"][n][k] for n in names]) for k in ev.TP_METRICS}
    nds = (5 * mean_ap + sum(1 - min(1, v) for v in errs.values())) / 10
    assert abs(r["nd_score"] - nds) < 1e-14
    own = ev.config_factory(class_names=["car"])
    assert abs(run(*dc.worked_case(), cfg=own)["mean_ap"] - r["mean_dist_aps"]["car"]) < 1e-15


def test_interp_equals_numpy():
    rs = np.random.RandomState(0)
    for n in (1, 2, 7, 300):
        xp = np.sort(rs.randint(0, max(2, n // 2), n) / max(2, n // 2))  # repeated values
        fp = rs.rand(n)
        x = np.concatenate([np.linspace(0, 1, 101), xp, [-1.0, 2.0]])
        np.testing.assert_allclose(ev.interp(x, xp, fp, right=0.0), np.interp(x, xp, fp, right=0), rtol=1e-13, atol=0)
        np.testing.assert_allclose(ev.interp(x, xp, fp), np.interp(x, xp, fp), rtol=1e-13, atol=0)
    # the curves of a case: the specification's tables against np.interp on the same cumulative arrays
    preds, gts = dc.random_case(5, 3, 5, 64, dc.CLASSES5)
    r = run(preds, gts)
    P, scores, p_cls, _ = ev.pack_preds_numpy(preds, CFG, dc.CLASSES5)
    _, g_cls, _ = ev.pack_gt(gts, CFG, dc.CLASSES5)
    order, off = ev.global_order(scores, p_cls, len(CFG.class_names))
    checked = 0
    for c in range(len(CFG.class_names)):
        o = order[off[c]:off[c + 1]]
        for t in range(4):
            flag = r["match"][t, o] >= 0
            if not flag.any():
                continue
            tp = np.cumsum(flag)
            rec, prec = tp / float((g_cls == c).sum()), tp / np.arange(1, o.size + 1)
            assert np.unique(rec).size < rec.size  # repeated recall values
            np.testing.assert_allclose(r["precision"][c, t], np.interp(np.linspace(0, 1, 101), rec, prec, right=0), rtol=1e-13)
            np.testing.assert_allclose(r["confidence"][c, t], np.interp(np.linspace(0, 1, 101), rec, scores[o], right=0), rtol=1e-13)
            checked += 1
    assert checked >= 4


def test_gt_conversion_two_float32_steps():
    z, dz = 0.1234567, 1.7654321
    g = ev.gt_lidar_boxes(np.array([[1, 2, z, 4, 2, dz, 0.3]]))
    zb = np.float32(np.float32(z) + np.float32(np.float32(dz) * np.float32(-0.5)))
    zc = np.float32(zb + np.float32(np.float32(dz) * np.float32(0.5)))
    assert g.dtype == np.float32 and g[0, 2] == zc and g.shape == (1, 9) and (g[0, 7:] == 0).all()
    p = ev.pred_lidar_boxes(np.array([[1, 2, z, 4, 2, dz, 0.3]], np.float32))
    assert p[0, 2] == np.float32(np.float32(z) + np.float32(np.float32(dz) * np.float32(0.5)))


def test_negative_gt_labels_are_dropped():
    p, g = one_sample([dc.box(0, 0), dc.box(0, 0)], [-1, 7], [dc.box(0, 0)], [0.5], [4])
    r = run(p, g)
    assert (r["match"] == -1).all() and r["label_aps"]["pedestrian"][2.0] == 0.0
    G, g_cls, g_off = ev.pack_gt(g, CFG, dc.CLASSES5)
    assert G.shape[0] == 0 and g_off.tolist() == [0, 0]


def test_invalid_inputs_raise():
    p, g = one_sample([dc.box(0, 0)], [0], [dc.box(0, 0)] * 501, [0.5] * 501, [0] * 501)
    with pytest.raises(ValueError, match="500"):
        run(p, g)
    with pytest.raises(ValueError, match="500"):
        ev.detection_eval(p, g, CFG, dc.CLASSES5)
    p, g = one_sample([dc.box(0, 0)], [0], [dc.box(0, 0)], [float("nan")], [0])
    with pytest.raises(ValueError, match="non-finite"):
        run(p, g)
    p, g = one_sample([dc.box(0, 0)], [0], [dc.box(float("inf"), 0)], [0.5], [0])
    with pytest.raises(ValueError, match="non-finite"):
        run(p, g)
    with pytest.raises(KeyError):
        run(*dc.worked_case(), classes=["car", "unicorn"])


def infos_and_results(n=4, device="cpu"):
    preds, gts = dc.random_case(11, n, 2, 20, dc.CLASSES5)
    infos = [dict(token="tok%d" % i, instances=[dict(bbox_3d=list(map(float, b)), bbox_label_3d=int(l)) for b, l in zip(*gts[i])])
             for i in range(n)]
    samples = [dict(pred_instances_3d=dict(bboxes_3d=torch.from_numpy(b).to(device), scores_3d=torch.from_numpy(s).to(device),
                                           labels_3d=torch.from_numpy(l).to(device)), sample_idx=i)
               for i, (b, s, l) in enumerate(preds)]
    return infos, samples, preds, gts


def test_metric_by_name(tmp_path):
    infos, samples, preds, gts = infos_and_results()
    ann = tmp_path / "infos.json"
    ann.write_text(json.dumps(dict(data_list=infos)))
    metric = METRICS.build(dict(type="NuScenesCustomMetric", data_root=str(tmp_path), ann_file="infos.json", metric="bbox"))
    assert metric.CLASSES == ("car", "truck", "bus", "bicycle", "pedestrian") and metric.ErrNameMapping["trans_err"] == "mATE"
    assert metric.DefaultAttribute["barrier"] == "" and metric.dataset_meta["classes"] == metric.CLASSES
    metric.process({}, samples[:2])
    metric.process({}, [dict(s["pred_instances_3d"], sample_idx=s["sample_idx"]) for s in samples[2:]])  # predict()'s dicts
    out = metric.compute_metrics(metric.results)
    want = run(preds, gts)
    assert out["mAP"] == want["mean_ap"] and out["NDS"] == want["nd_score"]
    for k in list(ev.TP_METRICS) + ["mAP_%s" % n for n in CFG.class_names]:
        assert k in out
    table = out["result"]
    assert table.startswith("----------------nuScenes default results-----------------\n")
    lines = table.split("\n")
    assert len(lines) == 3 + 5 and "AP@0.5m" in lines[1] and "error@trans_err" in lines[1] and "attr_err" not in lines[1]
    assert lines[3].startswith("| car") and ("%.2f" % (want["mean_dist_aps"]["car"] * 100)) in lines[3]
    assert metric.evaluate(4)["mAP"] == want["mean_ap"] and metric.results == []


def test_mismatched_sample_sets_raise():
    infos, samples, _, _ = infos_and_results()
    metric = METRICS.build(dict(type="NuScenesCustomMetric", data_list=infos))
    metric.process({}, samples[:3])
    with pytest.raises(AssertionError, match="Samples in split doesn't match samples in predictions."):
        metric.compute_metrics(metric.results)


def test_format_only_json(tmp_path):
    infos, samples, preds, _ = infos_and_results()
    metric = METRICS.build(dict(type="NuScenesCustomMetric", data_list=infos, format_only=True, jsonfile_prefix=str(tmp_path / "out")))
    metric.process({}, samples)
    assert metric.compute_metrics(metric.results) == {}
    doc = json.loads((tmp_path / "out" / "pred_instances_3d" / "results_nusc.json").read_text())
    assert set(doc) == {"meta", "results"} and set(doc["results"]) == {"tok%d" % i for i in range(4)}
    row, b = doc["results"]["tok0"][0], preds[0][0][0]
    assert set(row) == {"sample_token", "translation", "size", "rotation", "velocity", "detection_name", "detection_score",
                        "attribute_name"}
    assert row["size"] == [float(b[4]), float(b[3]), float(b[5])]
    assert row["rotation"] == [math.cos(float(b[6]) / 2), 0.0, 0.0, math.sin(float(b[6]) / 2)]
    assert row["translation"][2] == float(np.float32(b[2] + b[5] * np.float32(0.5)))
    assert row["detection_name"] == dc.CLASSES5[int(preds[0][2][0])]


def test_evaluate_tool(tmp_path, capsys):
    """tools/evaluate.py, in process: a results pickle and an ann file in, the table and the metrics JSON out."""
    import importlib.util
    import os
    import pickle
    spec = importlib.util.spec_from_file_location(
        "evaluate_tool", os.path.join(os.path.dirname(__file__), "..", "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    infos, samples, preds, gts = infos_and_results()
    (tmp_path / "infos.pkl").write_bytes(pickle.dumps(dict(data_list=infos)))
    (tmp_path / "results.pkl").write_bytes(pickle.dumps(
        [dict(sample_idx=i, bboxes_3d=b, scores_3d=s, labels_3d=l) for i, (b, s, l) in enumerate(preds)]))
    assert tool.main([str(tmp_path / "results.pkl"), str(tmp_path / "infos.pkl"), "--device", "cpu", "--json",
                      str(tmp_path / "m.json")]) == 0
    printed = capsys.readouterr().out
    want = run(preds, gts)
    assert "| car" in printed and ("mAP: %.4f" % want["mean_ap"]) in printed
    doc = json.loads((tmp_path / "m.json").read_text())
    assert doc["mean_ap"] == want["mean_ap"] and doc["nd_score"] == want["nd_score"] and doc["cfg"] == CFG.serialize()


def test_config_round_trip():
    assert CFG.class_names == ["car", "truck", "bus", "trailer", "construction_vehicle", "pedestrian", "motorcycle", "bicycle",
                               "traffic_cone", "barrier"]
    assert CFG.class_range["pedestrian"] == 40 and CFG.class_range["barrier"] == 30 and CFG.class_range["car"] == 50
    assert (CFG.dist_ths, CFG.dist_th_tp, CFG.min_recall, CFG.min_precision) == ([0.5, 1.0, 2.0, 4.0], 2.0, 0.1, 0.1)
    assert (CFG.max_boxes_per_sample, CFG.mean_ap_weight, CFG.dist_fcn) == (500, 5, "center_distance")
    again = ev.DetectionConfig.deserialize(json.loads(json.dumps(CFG.serialize())))
    assert again == CFG and again.serialize() == CFG.serialize()
    with pytest.raises(ValueError):
        ev.config_factory("other")


def test_cpu_tensors_take_the_specification():
    preds, gts = dc.random_case(3, 2, 3, 10, dc.CLASSES5)
    before = dict(ev.PATHS)
    r = ev.detection_eval([tuple(torch.from_numpy(a) for a in p) for p in preds], gts, CFG, dc.CLASSES5)
    assert ev.PATHS["torch"] == before["torch"] + 1 and ev.PATHS["kernel"] == before["kernel"]
    assert r["mean_ap"] == run(preds, gts)["mean_ap"]
