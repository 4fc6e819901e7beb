#!/usr/bin/env python3
"""Writes tests/golden/gt_database.npz: the reference's own create_groundtruth_database (tools/dataset_converters/
create_gt_database.py:111-340) on four small synthetic frames, for tests/test_gt_database_cpu.py and
tests/test_points_in_boxes_gpu.py.

The reference is loaded at run time from REFERENCE_ROOT (default /root/reference) behind the stubs of
make_object_sample_golden.py (numba as an identity jit; mmcv, mmengine, mmdet as stub modules) plus pycocotools; nothing of it
is copied.  The function itself runs: `DATASETS.build` returns a small in-memory object with `get_data_info`, `pipeline` (the
points as a tensor, `ann_info` with the boxes as a tensor: both have the `.numpy()` the loop calls) and `metainfo`, mmengine's
mkdir_or_exist / track_iter_progress are os.makedirs / the identity.  Recorded: the bytes of every file it writes, the file
names, every field of the info pickle, and box_np_ops.points_in_rbbox's mask per frame.

Frames: three with C = 5 and 400-800 points, one with C = 3; 5-12 boxes each, centred on clusters of the cloud.  In every frame
boxes 0 and 1 overlap (asserted: some points are in both) and the last box holds nothing; frame 1 has 9-column boxes; frame 0
alone has group_ids (with repeats), difficulty and score; frame 2 has one row with a NaN x, which is inside every box (asserted),
the empty one included; USED leaves the class 'barrier' out, so its files are written and its infos are not.

As in the ObjectSample fixture every point with a plane sign closer to zero than 4 * 2^-24 * (|x n0| + |y n1| + |z n2| + |d|), the
rounding bound of the four-term float32 sum, is taken out of the input before anything is recorded, so any evaluation order
gives the same mask; fewer than 5 % of the points go that way (asserted: a condition on the inputs, not a tolerance)."""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_object_sample_golden as base  # noqa: E402  the stubs and the loader of the reference's modules

CLASSES = ["car", "pedestrian", "truck", "barrier"]
USED = ["car", "pedestrian", "truck"]
FRAMES = ((640, 5, 9, 7), (480, 5, 12, 9), (760, 5, 6, 7), (420, 3, 5, 7))  # points, C, boxes, box columns
PREFIX = "golden"


def make_frame(rs, n, C, K, cols):
    centres = np.concatenate([rs.uniform(-25, 25, (K, 2)), rs.uniform(-1.5, 0.5, (K, 1))], 1)
    centres[1, :2] = centres[0, :2] + [0.9, -0.6]            # boxes 0 and 1 overlap
    centres[K - 1, :2] = [47.0, 46.0]                        # the last box: no point is near it
    dims = rs.uniform([1.8, 1.2, 1.2], [4.8, 2.4, 2.2], (K, 3))
    boxes = np.concatenate([centres - [0, 0, 1.0], dims, rs.uniform(-np.pi, np.pi, (K, 1)), rs.uniform(-3, 3, (K, cols - 7))], 1)
    near = centres[rs.randint(0, K - 1, int(0.6 * n))]
    clustered = near + rs.normal(scale=[1.1, 1.1, 0.6], size=near.shape)
    spread = np.concatenate([rs.uniform(-30, 30, (n - len(near), 2)), rs.uniform(-3, 1.5, (n - len(near), 1))], 1)
    xyz = np.concatenate([clustered, spread], 0)[rs.permutation(n)]
    pts = np.concatenate([xyz, rs.rand(n, C - 3)], 1).astype(np.float32)
    labels = rs.randint(0, len(CLASSES), K).astype(np.int64)
    labels[:4] = [0, 3, 1, 2]  # every class in every frame, the one left out among them
    return pts, boxes.astype(np.float32), labels


class Dataset:
    """What the reference's loop needs of a dataset."""

    def __init__(self, frames):
        self.frames, self.metainfo = frames, dict(classes=CLASSES)

    def __len__(self):
        return len(self.frames)

    def get_data_info(self, j):
        return self.frames[j]

    def pipeline(self, info):
        ann = dict(info["ann_info"], gt_bboxes_3d=torch.from_numpy(info["ann_info"]["gt_bboxes_3d"].copy()))
        return dict(sample_idx=info["sample_idx"], points=torch.from_numpy(info["points"].copy()), ann_info=ann)


def load_builder(frames):
    _, _, ops, _ = base.load_reference()
    for name in ("mmcv.ops", "mmdet.evaluation", "pycocotools", "pycocotools.mask", "pycocotools.coco"):
        base._stub(name)
    base._stub("mmengine", print_log=lambda *a, **k: None, track_iter_progress=lambda it: it,
               mkdir_or_exist=lambda d: os.makedirs(d, exist_ok=True))
    sys.modules["mmdet3d.registry"].DATASETS = type("DATASETS", (), {"build": staticmethod(lambda cfg: Dataset(frames))})
    mod = base._load("create_gt_database", "tools/dataset_converters/create_gt_database.py")
    return ops, mod


def main():
    rs = np.random.RandomState(29)
    frames, removed, total = [], 0, 0
    ops, mod = load_builder(frames)  # the dataset is built when the reference asks for it, from the list as it is then
    for f, (n, C, K, cols) in enumerate(FRAMES):
        pts, boxes, labels = make_frame(rs, n, C, K, cols)
        ok = base.margins_ok(ops, pts, boxes)
        removed, total = removed + int((~ok).sum()), total + n
        pts = np.ascontiguousarray(pts[ok])
        if f == 2:
            pts[len(pts) // 3, 0] = np.nan
        ann = dict(gt_bboxes_3d=boxes, gt_labels_3d=labels)
        if f == 0:
            ann.update(group_ids=np.array([0, 0, 1, 2, 2, 3, 7, 7, 5][:K], np.int64), difficulty=rs.randint(0, 3, K).astype(np.int64),
                       score=rs.rand(K))
        frames.append(dict(sample_idx=100 + 7 * f, points=pts, ann_info=ann))
    print("points within the rounding bound of a plane, taken out: %d of %d" % (removed, total))
    assert removed < 0.05 * total

    out = dict(classes=np.array(CLASSES), used_classes=np.array(USED), n_frames=np.array(len(frames)), info_prefix=np.array(PREFIX))
    for f, fr in enumerate(frames):
        mask = ops.points_in_rbbox(fr["points"], fr["ann_info"]["gt_bboxes_3d"])
        finite = np.isfinite(fr["points"][:, 0])
        assert (mask[finite, 0] & mask[finite, 1]).any(), "frame %d: boxes 0 and 1 share no point" % f
        assert not mask[finite, -1].any() and mask[finite, :-1].any(0).all(), "frame %d: which boxes hold points" % f
        assert mask[~finite].all(), "a NaN row is inside every box"
        assert (f == 2) == bool((~finite).any())
        key = "frame%d_" % f
        out[key + "points"], out[key + "mask"], out[key + "sample_idx"] = fr["points"], mask, np.array(fr["sample_idx"])
        for k, v in fr["ann_info"].items():
            out[key + k] = v
        print("frame %d: %d points, members per box %s" % (f, len(fr["points"]), mask.sum(0).tolist()))

    with tempfile.TemporaryDirectory() as root:
        mod.create_groundtruth_database("InMemoryDataset", root, PREFIX, used_classes=USED)
        db = os.path.join(root, PREFIX + "_gt_database")
        names = sorted(os.listdir(db))
        blobs = [np.fromfile(os.path.join(db, name), dtype=np.uint8) for name in names]
        with open(os.path.join(root, PREFIX + "_dbinfos_train.pkl"), "rb") as fh:
            infos = pickle.load(fh)
    assert len(names) == sum(fr[2] for fr in FRAMES) and "barrier" not in infos and any("barrier" in name for name in names)
    out["file_names"], out["file_sizes"] = np.array(names), np.array([len(b) for b in blobs])
    out["file_bytes"] = np.concatenate(blobs)
    flat = [info for name in infos for info in infos[name]]
    out["info_classes"] = np.array(list(infos))                       # the pickle's key order
    out["info_class_sizes"] = np.array([len(infos[name]) for name in infos])
    assert all(sorted(info) == sorted(["name", "path", "image_idx", "gt_idx", "box3d_lidar", "num_points_in_gt", "difficulty",
                                       "group_id"] + (["score"] if info["image_idx"] == 100 else [])) for info in flat)
    for field in ("name", "path", "image_idx", "gt_idx", "num_points_in_gt", "difficulty", "group_id"):
        out["info_" + field] = np.array([info[field] for info in flat])
    out["info_difficulty_dtype"] = np.array([np.asarray(info["difficulty"]).dtype.str for info in flat])
    assert all(info["box3d_lidar"].dtype == np.float32 for info in flat)
    out["info_box_cols"] = np.array([len(info["box3d_lidar"]) for info in flat])
    out["info_boxes"] = np.concatenate([info["box3d_lidar"] for info in flat])
    out["info_score"] = np.array([info.get("score", np.nan) for info in flat], np.float64)
    path = os.path.join(HERE, "gt_database.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(names), "files,", len(flat), "infos")


if __name__ == "__main__":
    main()
