#!/usr/bin/env python3
"""Writes tests/golden/points_aug.npz: the reference's own LiDAR augmentation chain (BEVFusionGlobalRotScaleTrans or
GlobalRotScaleTrans, BEVFusionRandomFlip3D, PointsRangeFilter, ObjectRangeFilter, ObjectNameFilter) on seeded inputs, for
tests/test_points_aug_cpu.py and tests/test_points_aug_gpu.py.

The reference's classes are loaded at run time from REFERENCE_ROOT (default /root/reference) behind stubs of the packages that
are not installed (cv2, mmcv, mmengine, mmdet and the parts of mmdet3d the chain does not touch); nothing of it is copied.  Real
files, in this order: mmdet3d/utils/array_converter.py, structures/bbox_3d/utils.py, structures/points/{base,lidar}_points.py,
structures/bbox_3d/{base,lidar}_box3d.py, datasets/transforms/transforms_3d.py, projects/BEVFusion/bevfusion/transforms_3d.py.

Inputs: N_POINTS seeded points [n, 5] spread over +-65 m (about half outside +-54 m), 12 boxes [12, 9] with labels, some out of
range and two with a label no class has.  Draws: TRAIN_SEEDS with the lidar-cam config's parameters (every flip combination
occurs: asserted), one with the plain GlobalRotScaleTrans, one without boxes (the einsum path) and the test pipeline
(PointsRangeFilter only).  After each draw the next np.random.uniform() is recorded, so a restatement can be held to the same
number of generator calls.

Also asserted: no transformed coordinate lies within 12 * 2^-24 * s * (|x| + |y| + |z| + |t_c|) of a face of the range, the bound
the tests allow between two float32 evaluations of the chain, so the kept mask of any such evaluation is the reference's."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
N_POINTS = 2000
RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
           "traffic_cone"]
GRST = dict(rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5])
TRAIN_SEEDS = (0, 2, 3, 4)
# (kind, seed): "bev" the BEVFusion chain, "plain" GlobalRotScaleTrans in its place, "noboxes" the BEVFusion chain on points
# alone, "test" PointsRangeFilter only
DRAWS = [("bev", s) for s in TRAIN_SEEDS] + [("plain", 11), ("noboxes", 12), ("test", 0)]


class _Any(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (object,), {})


class _Registry:
    def register_module(self, *a, **k):
        return lambda cls: cls


def _stub(name, **attrs):
    mod = _Any(name)
    mod.__dict__.update(attrs)
    mod.__path__ = []
    sys.modules[name] = mod
    return mod


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ("cv2", "mmcv", "mmcv.transforms", "mmcv.ops", "mmdet", "mmdet.datasets", "mmdet.datasets.transforms", "mmengine",
                 "mmdet3d", "mmdet3d.models", "mmdet3d.models.task_modules", "mmdet3d.structures", "mmdet3d.structures.ops",
                 "mmdet3d.structures.bbox_3d", "mmdet3d.datasets", "mmdet3d.datasets.transforms",
                 "mmdet3d.datasets.transforms.data_augment_utils"):
        _stub(name)
    _stub("mmdet3d.registry", TRANSFORMS=_Registry())
    ac = _load("mmdet3d.utils.array_converter", "mmdet3d/utils/array_converter.py")
    _stub("mmdet3d.utils", array_converter=ac.array_converter)
    _load("mmdet3d.structures.bbox_3d.utils", "mmdet3d/structures/bbox_3d/utils.py")
    bp = _load("mmdet3d.structures.points.base_points", "mmdet3d/structures/points/base_points.py")
    lp = _load("mmdet3d.structures.points.lidar_points", "mmdet3d/structures/points/lidar_points.py")
    _stub("mmdet3d.structures.points", BasePoints=bp.BasePoints, LiDARPoints=lp.LiDARPoints)
    _load("mmdet3d.structures.bbox_3d.base_box3d", "mmdet3d/structures/bbox_3d/base_box3d.py")
    lb = _load("mmdet3d.structures.bbox_3d.lidar_box3d", "mmdet3d/structures/bbox_3d/lidar_box3d.py")
    sys.modules["mmdet3d.structures"].LiDARInstance3DBoxes = lb.LiDARInstance3DBoxes
    sys.modules["mmdet3d.structures"].BasePoints = bp.BasePoints
    t3 = _load("mmdet3d.datasets.transforms.transforms_3d", "mmdet3d/datasets/transforms/transforms_3d.py")
    sys.modules["mmdet3d.datasets"].GlobalRotScaleTrans = t3.GlobalRotScaleTrans
    bf = _load("reference_bevfusion_transforms_3d", "projects/BEVFusion/bevfusion/transforms_3d.py")
    return lp.LiDARPoints, lb.LiDARInstance3DBoxes, t3, bf


def inputs():
    rs = np.random.RandomState(5)
    pts = ((rs.rand(N_POINTS, 5) - 0.5) * np.array([130, 130, 10, 1, 1])).astype(np.float32)
    boxes = ((rs.rand(12, 9) - 0.5) * np.array([120, 120, 4, 4, 4, 4, 6, 10, 10])).astype(np.float32)
    boxes[:, 3:6] = np.abs(boxes[:, 3:6]) + 0.5
    labels = (np.arange(12) % 11 - 1).astype(np.int64)  # -1 twice: no class
    return pts, boxes, labels


def bound(pts, scale, trans):
    """[n, 3]: the tests' tolerance per coordinate."""
    mag = np.abs(pts[:, :3].astype(np.float64)).sum(1, keepdims=True) + np.abs(np.asarray(trans, np.float64))[None, :]
    return 12.0 * 2.0 ** -24 * float(scale) * mag


def main():
    LiDARPoints, Boxes, t3, bf = load_reference()
    pts, boxes, labels = inputs()
    out = dict(points=pts, boxes=boxes, labels=labels, point_cloud_range=np.array(RANGE, np.float32),
               n_classes=np.array(len(CLASSES)))
    flips_seen = set()
    for d, (kind, seed) in enumerate(DRAWS):
        data = dict(points=LiDARPoints(torch.from_numpy(pts.copy()), points_dim=5))
        if kind in ("bev", "plain"):
            data["gt_bboxes_3d"] = Boxes(torch.from_numpy(boxes.copy()), box_dim=9)
            data["gt_labels_3d"] = labels.copy()
        np.random.seed(seed)
        flips = (0, 0)
        if kind != "test":
            cls = t3.GlobalRotScaleTrans if kind == "plain" else bf.BEVFusionGlobalRotScaleTrans
            data = cls(**GRST).transform(data)
            state = np.random.get_state()
            data = bf.BEVFusionRandomFlip3D()(data)
            after = np.random.get_state()
            np.random.set_state(state)  # replay the flip's two draws to learn them
            flips = (int(np.random.choice([0, 1])), int(np.random.choice([0, 1])))
            assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), after))
            if kind == "bev":
                flips_seen.add(flips)
        full = data["points"].tensor.numpy().copy()  # transformed, before the filter
        data = t3.PointsRangeFilter(point_cloud_range=RANGE).transform(data)
        if "gt_bboxes_3d" in data:
            data = t3.ObjectRangeFilter(point_cloud_range=RANGE).transform(data)
            data = t3.ObjectNameFilter(classes=CLASSES).transform(data)
        nxt = np.random.uniform()

        scale = data.get("pcd_scale_factor", 1.0)
        trans = data.get("pcd_trans", np.zeros(3))
        rng = np.array(RANGE, np.float32).astype(np.float64)
        margin = np.minimum(np.abs(full[:, :3].astype(np.float64) - rng[None, :3]), np.abs(full[:, :3].astype(np.float64) - rng[None, 3:]))
        assert (margin > bound(pts, scale, trans)).all(), "draw %d: a coordinate within the tolerance of a range face" % d
        mask = ((full[:, :3] > rng[None, :3]) & (full[:, :3] < rng[None, 3:])).all(1)
        kept = data["points"].tensor.numpy()
        assert np.array_equal(full[mask], kept)

        out["draw%d_kind" % d] = np.array(kind)
        out["draw%d_seed" % d] = np.array(seed)
        out["draw%d_angle" % d] = np.array(data.get("pcd_rotation_angle", 0.0), np.float64)
        out["draw%d_scale" % d] = np.array(scale, np.float64)
        out["draw%d_trans" % d] = np.asarray(trans, np.float64)
        out["draw%d_rotation" % d] = data["pcd_rotation"].numpy() if "pcd_rotation" in data else np.eye(3, dtype=np.float32)
        out["draw%d_flips" % d] = np.array(flips, np.int64)
        out["draw%d_matrix" % d] = np.asarray(data.get("lidar_aug_matrix", np.eye(4)), np.float64)
        out["draw%d_flow" % d] = np.array("".join(data.get("transformation_3d_flow", [])))
        out["draw%d_mask" % d] = mask
        out["draw%d_xyz" % d] = kept[:, :3]  # columns 3 .. are points[mask][:, 3:], unchanged
        assert np.array_equal(kept[:, 3:], pts[mask][:, 3:])
        if "gt_bboxes_3d" in data:
            out["draw%d_boxes" % d] = data["gt_bboxes_3d"].tensor.numpy()
            out["draw%d_labels" % d] = np.asarray(data["gt_labels_3d"])
        out["draw%d_next_uniform" % d] = np.array(nxt, np.float64)
        assert 0.3 * N_POINTS < mask.sum() < 0.8 * N_POINTS, mask.sum()
    assert flips_seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, "flip combinations seen: %s -- choose other seeds" % sorted(flips_seen)
    out["n_draws"] = np.array(len(DRAWS))
    path = os.path.join(HERE, "points_aug.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
