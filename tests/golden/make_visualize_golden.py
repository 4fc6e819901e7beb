#!/usr/bin/env python3
"""Writes tests/golden/visualize_ref.npz for tests/test_visualize_cpu.py: what the reference's own visualisation tool computes.

The reference's `project_to_image`, `Track` and `Tracker3D` (tools/visualize/visualize_bboxes_bevfusion.py:55-160) are taken out
of the file under REFERENCE_ROOT (default /root/reference) at run time -- the three definitions are cut from its syntax tree and
executed with numpy and scipy, since the file itself imports cv2, matplotlib and mmengine at its top; nothing of it is copied.

(a) Projection.  The six cameras of tests/golden/jpeg_cases.npz (`transform_out_lidar2cam`, `transform_out_ori_cam2img`, the
    matrices BEVLoadMultiViewImageFromFiles records), rounded to float32 first so that the reference sees the values the package
    sees.  Twelve boxes on a ring round the vehicle, 5 to 31 m out, so that each camera has boxes in front of it, beside it and
    behind it, and two long boxes close to the vehicle that lie ACROSS the image planes of several cameras (asserted below: for
    every camera at least one box with all corners in front, one with all behind and one with both).  Recorded: the float64
    corners, `project_to_image`'s float64 pixels (its `+ 1e-8` in the divisor included) and its validity flags, and z_cam.
    LiDARInstance3DBoxes does not load without mmcv's compiled ops, so the corners are the RESTATED formula of
    lidar_box3d.py:41-80 in float64 (unit corners, times dims, rotated about z, plus the bottom centre).
    No corner of any box lies within 1e-3 m of any camera's plane z_cam = 0 (asserted), four orders above the float32 rounding
    bound of z_cam at these magnitudes, so the validity flags are the same in any arithmetic.
(b) Tracker.  Eight frames of detections [x, y, z, dx, dy, dz, yaw, score, label] through one Tracker3D(max_missed=3,
    max_dist=4.0): frame 1 has a detection of another class 0.2 m from a track (a new track, not a match) and one 4.5 m from its
    track (beyond max_dist: a new track); the tracks left behind are missed in frames 1, 2, 3 -- frame 3 is EMPTY -- and a
    fourth time in frame 4, where they leave; frame 5 puts a detection where a track left (a new id); frame 7 has two
    detections of one class near one track.  Recorded per frame: the ids and boxes of get_results()."""
import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
TOOL = os.path.join(REF, "tools", "visualize", "visualize_bboxes_bevfusion.py")


def load_reference():
    from typing import List, Optional
    from scipy.optimize import linear_sum_assignment
    text = open(TOOL).read()
    ns = dict(np=np, List=List, Optional=Optional, linear_sum_assignment=linear_sum_assignment)
    for node in ast.parse(text).body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in ("Track", "Tracker3D", "project_to_image"):
            exec(compile(ast.Module([node], []), TOOL, "exec"), ns)
    return ns["project_to_image"], ns["Tracker3D"]


def corners64(boxes):
    unit = np.stack(np.unravel_index(np.arange(8), [2, 2, 2]), 1)[[0, 1, 3, 2, 4, 5, 7, 6]] - np.array([0.5, 0.5, 0.0])
    b = boxes.astype(np.float64)
    loc = b[:, None, 3:6] * unit[None]
    c, s = np.cos(b[:, None, 6]), np.sin(b[:, None, 6])
    return np.stack([loc[..., 0] * c - loc[..., 1] * s + b[:, None, 0], loc[..., 0] * s + loc[..., 1] * c + b[:, None, 1],
                     loc[..., 2] + b[:, None, 2]], -1)


def make_boxes():
    rs = np.random.RandomState(7)
    ang = np.deg2rad(np.arange(12) * 30.0 + 7.0)
    rad = rs.uniform(5.0, 31.0, 12)
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang), rs.uniform(-2.0, -0.5, 12), rs.uniform(1.5, 5.0, 12),
                     rs.uniform(0.6, 2.2, 12), rs.uniform(1.0, 2.5, 12), rs.uniform(-np.pi, np.pi, 12)], 1)
    across = np.array([[1.5, 0.7, -1.6, 14.0, 2.4, 2.0, 0.3], [-0.9, 1.1, -1.4, 11.0, 2.0, 1.8, 1.9]])
    return np.concatenate([ring, across], 0).astype(np.float32)


def tracker_frames():
    def det(x, y, label, score=0.6):
        return [x, y, -1.0, 4.0, 1.9, 1.6, 0.25, score, label]
    frames = [
        [det(0, 0, 0), det(10, 0, 8), det(20, 5, 1)],
        [det(1, 0, 0), det(10.2, 0, 0), det(20, 9.5, 1)],
        [det(2, 0, 0)],
        [],
        [det(3, 0, 0)],
        [det(4, 0, 0), det(10, 0, 8)],
        [det(5, 0, 0), det(10.5, 0.5, 8)],
        [det(6, 0, 0), det(6.5, 3, 0), det(11, 1, 8)],
    ]
    return [np.array(f, np.float32).reshape(-1, 9) for f in frames]


def main():
    project_to_image, Tracker3D = load_reference()
    cal = np.load(os.path.join(HERE, "jpeg_cases.npz"))
    lidar2cam = cal["transform_out_lidar2cam"].astype(np.float32)
    cam2img = cal["transform_out_ori_cam2img"].astype(np.float32)
    boxes = make_boxes()
    corners = corners64(boxes)
    n, N = boxes.shape[0], lidar2cam.shape[0]
    uv = np.zeros((N, n, 8, 2))
    valid = np.zeros((N, n, 8), bool)
    z_cam = np.zeros((N, n, 8))
    for c in range(N):
        for i in range(n):
            uv[c, i], valid[c, i] = project_to_image(corners[i], lidar2cam[c].astype(np.float64), cam2img[c].astype(np.float64))
            z_cam[c, i] = (lidar2cam[c].astype(np.float64) @ np.concatenate([corners[i], np.ones((8, 1))], 1).T)[2]
    assert np.abs(z_cam).min() > 1e-3, np.abs(z_cam).min()
    assert np.array_equal(valid, z_cam > 0)
    for c in range(N):
        assert valid[c].all(1).any() and (~valid[c]).all(1).any() and (valid[c].any(1) & ~valid[c].all(1)).any(), c

    tracker = Tracker3D(max_missed=3, max_dist=4.0)
    frames = tracker_frames()
    ids, out_boxes, out_off = [], [], [0]
    for f in frames:
        res = tracker.update(f if len(f) else np.zeros((0, 9), np.float32))
        ids += [r["id"] for r in res]
        out_boxes += [r["box"] for r in res]
        out_off.append(len(ids))
    per = [ids[a:b] for a, b in zip(out_off[:-1], out_off[1:])]
    assert per[1] == [1, 2, 3, 4, 5] and per[3] == [1, 2, 3, 4, 5] and per[4] == [1, 4, 5] and per[5] == [1, 6], per
    np.savez_compressed(
        os.path.join(HERE, "visualize_ref.npz"), boxes=boxes, lidar2cam=lidar2cam, cam2img=cam2img, corners=corners, uv=uv,
        valid=valid, z_cam=z_cam, trk_dets=np.concatenate(frames, 0), trk_det_off=np.cumsum([0] + [len(f) for f in frames]),
        trk_ids=np.array(ids, np.int64), trk_boxes=np.array(out_boxes, np.float32).reshape(-1, 9), trk_off=np.array(out_off, np.int64))
    print("wrote visualize_ref.npz: %d boxes, %d cameras, tracker ids per frame %s" % (n, N, per))


if __name__ == "__main__":
    main()
