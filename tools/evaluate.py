#!/usr/bin/env python3
"""nuScenes-protocol evaluation of saved predictions: a results pickle plus an annotation file in, the per-class table out.

    evaluate.py RESULTS.pkl ANN_FILE [--classes car,truck,...] [--device cuda:0|cpu] [--json OUT.json] [--format-only DIR]

RESULTS.pkl: a list with one entry per sample, each {'sample_idx': i, 'pred_instances_3d': {'bboxes_3d', 'scores_3d',
'labels_3d'}} or {'sample_idx', 'bboxes_3d', 'scores_3d', 'labels_3d'} (tensors or arrays; boxes [n, 7 or 9] in LiDAR
convention with the bottom centre) -- what NuScenesCustomMetric.process collects.  ANN_FILE: the infos (.pkl or .json with a
`data_list`).  With --device cuda:0 (the default when a GPU is present) the predictions are moved to the device and the HIP
kernels evaluate them; with cpu the numpy specification does, same numbers.  --json writes the metrics (the devkit's
metrics_summary keys); --format-only writes results_nusc.json under DIR instead of evaluating."""
import argparse
import json
import os
import pickle
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import evaluation as ev
from bevfusion_amd.registry import METRICS


def to_device(x, dev):
    x = getattr(x, "tensor", x)
    return (x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("results")
    ap.add_argument("ann_file")
    ap.add_argument("--classes", default=None, help="comma-separated class names of the labels (default: the metric's CLASSES)")
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--json", default=None)
    ap.add_argument("--format-only", default=None, metavar="DIR")
    args = ap.parse_args(argv)
    with open(args.results, "rb") as f:
        results = pickle.load(f)
    metric = METRICS.build(dict(type="NuScenesCustomMetric", ann_file=args.ann_file, format_only=args.format_only is not None,
                                jsonfile_prefix=args.format_only))
    if args.classes:
        metric.CLASSES = tuple(args.classes.split(","))
        metric.dataset_meta = dict(metric.dataset_meta, classes=metric.CLASSES)
    dev = torch.device(args.device)
    samples = []
    for r in results:
        p = r.get("pred_instances_3d", r)
        samples.append(dict(sample_idx=r["sample_idx"], bboxes_3d=to_device(p["bboxes_3d"], dev).float(),
                            scores_3d=to_device(p["scores_3d"], dev).float(), labels_3d=to_device(p["labels_3d"], dev)))
    metric.process({}, samples)
    out = metric.evaluate(len(samples))
    if args.format_only is not None:
        print("results written under %s" % args.format_only)
        return 0
    print(out["result"])
    print("mAP: %.4f  NDS: %.4f  (%s path)" % (out["mAP"], out["NDS"], "kernel" if ev.PATHS["kernel"] else "host"))
    if args.json:
        keep = {k: v for k, v in out["metrics"].items() if k in ("label_aps", "mean_dist_aps", "mean_ap", "label_tp_errors", "tp_errors",
                                                                  "tp_scores", "nd_score", "cfg")}
        keep["label_aps"] = {n: {str(k): v for k, v in d.items()} for n, d in keep["label_aps"].items()}
        with open(args.json, "w") as f:
            json.dump(keep, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
