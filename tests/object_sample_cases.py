"""Shared by tests/test_object_sample_cpu.py and tests/test_object_sample_gpu.py: the recorded reference draws of ObjectSample
(tests/golden/object_sample.npz, written by tests/golden/make_object_sample_golden.py), the database rebuilt from the fixture
as the files DataBaseSampler reads, and this package's transform on the same inputs."""
import os
import pickle

import numpy as np
import torch

from bevfusion_amd import points_aug as pa  # noqa: F401  registers the transforms
from bevfusion_amd.registry import TRANSFORMS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "object_sample.npz")

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def n_draws():
    return len(golden()["seeds"])


def n_calls():
    return int(golden()["calls"])


def write_database(root):
    """The fixture's database under `root` (a pickle of infos + one .bin per object) -> the db_sampler config."""
    g = golden()
    classes = [str(c) for c in g["classes"]]
    infos = {name: [] for name in classes}
    starts = np.concatenate([[0], np.cumsum(g["db_counts"])])
    os.makedirs(os.path.join(str(root), "db"), exist_ok=True)
    for i, c in enumerate(g["db_class"]):
        rel = "db/%d_%s.bin" % (i, classes[c])
        g["db_points"][starts[i]:starts[i + 1]].tofile(os.path.join(str(root), rel))
        infos[classes[c]].append(dict(name=classes[c], path=rel, box3d_lidar=g["db_boxes"][i].copy(),
                                      num_points_in_gt=int(g["db_num_points_in_gt"][i]), difficulty=int(g["db_difficulty"][i])))
    info_path = os.path.join(str(root), "dbinfos.pkl")
    with open(info_path, "wb") as f:
        pickle.dump(infos, f)
    load_dim = int(g["load_dim"])
    return dict(data_root=str(root), info_path=info_path, rate=1.0,
                prepare=dict(filter_by_difficulty=[-1], filter_by_min_points={name: int(g["min_points"]) for name in classes}),
                classes=classes, sample_groups={str(k): int(v) for k, v in zip(g["group_names"], g["group_nums"])},
                points_loader=dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=load_dim, use_dim=list(range(load_dim))))


def frame(arrays=False):
    g = golden()
    pts, boxes, labels = g["points"].copy(), g["gt_boxes"].copy(), g["gt_labels"].copy()
    if arrays:
        return dict(points=pts, gt_bboxes_3d=boxes, gt_labels_3d=labels)
    return dict(points=torch.from_numpy(pts), gt_bboxes_3d=torch.from_numpy(boxes), gt_labels_3d=labels)


def run(cfg, d, defer=False, arrays=False, after=()):
    """Draw d: np.random.seed, build ObjectSample (+ the transforms `after`, dicts), n_calls() frames through them ->
    ([data per call], the next np.random.uniform())."""
    np.random.seed(int(golden()["seeds"][d]))
    steps = [TRANSFORMS.build(dict(type="ObjectSample", db_sampler=dict(cfg), defer=defer))] + [TRANSFORMS.build(s) for s in after]
    out = []
    for _ in range(n_calls()):
        data = frame(arrays)
        for t in steps:
            data = t.transform(data)
        out.append(data)
    return out, np.random.uniform()


def reference(d, c):
    """(sampled boxes, labels, the reference's output points) of call c of draw d."""
    g = golden()
    key = "draw%d_call%d_" % (d, c)
    return g[key + "boxes"], g[key + "labels"], np.concatenate([g[key + "pasted"], g["points"][~g[key + "mask"]]], 0)
