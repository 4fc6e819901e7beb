#!/usr/bin/env python3
"""Points in rotated boxes, per box, on the device: csrc/points_in_boxes.hip (box_ops.points_in_boxes) against its plain-torch
specification on the GPU and a vectorised numpy restatement on one host core.

Shape: one nuScenes-shaped sample, POINTS = 260 000 rows over +-65 m, C = 5, already on the device; BOXES = 40 and then 130 boxes
of class-typical sizes (car, truck, bus, trailer, pedestrian, motorcycle, bicycle, barrier, cone) centred on points of the
cloud, a fresh draw of boxes per call, made before the timed window.  Per box count one JSON entry:

  kernel    box_ops.points_in_boxes(center=True): the planes on the host, packing planes and centres into one pinned buffer,
            ONE host-to-device copy, the count and scan launches, the host read of the K counts, the gather launch, the
            allocations -- the call as the builder makes it.  A host clock around CALLS calls; median of TIMED windows after
            WARMUP, alternating with the torch window, window by window.
  torch     box_ops.torch_points_in_boxes(center=True) on the same device tensor (the fallback path).
  host      numpy on ONE thread: per box and plane ((x n0 + y n1) + z n2) + d >= 0 over all rows, then the gather and the
            centring per box.  Median over HOST_REPEATS draws.

The kernel's and the specification's outputs are compared bit for bit first, the numpy masks with them.  A missing GPU is an
error.  Usage: gt_database_micro.py [OUT.json]   (default OUT: profiles/gt_database_micro.json)"""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import box_ops
from bevfusion_amd import points_aug as pa

POINTS, C = 260000, 5
BOX_COUNTS = (40, 130)
SIZES = np.array([[4.6, 1.9, 1.7], [6.9, 2.5, 2.8], [11.0, 2.9, 3.5], [12.3, 2.9, 3.9], [0.7, 0.7, 1.8], [2.1, 0.8, 1.5],
                  [1.7, 0.6, 1.3], [2.5, 0.5, 1.0], [0.4, 0.4, 1.1]], np.float32)
CALLS, WARMUP, TIMED = 5, 3, 20
HOST_REPEATS = 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def draw_boxes(rs, cloud, K):
    at = cloud[rs.randint(0, len(cloud), K), :3]
    dims = SIZES[rs.randint(0, len(SIZES), K)] * rs.uniform(0.9, 1.1, (K, 3))
    return np.concatenate([at - dims[:, 2:3] * np.array([[0, 0, 0.5]]), dims, rs.uniform(-np.pi, np.pi, (K, 1)), rs.normal(size=(K, 2))],
                          1).astype(np.float32)


def numpy_points_in_boxes(points, boxes):
    """(counts, centred rows, mask [n, K]) in vectorised numpy."""
    planes = pa.paste_planes(boxes)
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    mask = np.ones((len(points), len(boxes)), bool)
    rows = []
    for j in range(len(boxes)):
        left = np.zeros(len(points), bool)
        for k in range(6):
            n0, n1, n2, d = planes[j, k]
            left |= (((x * n0 + y * n1) + z * n2) + d) >= 0
        mask[:, j] = ~left
        r = points[mask[:, j]]
        r[:, :3] -= boxes[j, :3]
        rows.append(r)
    return mask.sum(0).astype(np.int32), np.concatenate(rows, 0), mask


def host_clock(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(dev, K, host, points):
    n_draws = (WARMUP + TIMED) * CALLS
    rs = np.random.RandomState(K)
    drawn = [draw_boxes(rs, host, K) for _ in range(n_draws)]
    state = {"i": 0}

    def next_boxes():
        b = drawn[state["i"] % n_draws]
        state["i"] += 1
        return b

    assert box_ops.ENABLED and box_ops.kernel_supported(points, K)
    a = box_ops.points_in_boxes(points, drawn[0], center=True, return_mask=True)
    b = box_ops.torch_points_in_boxes(points, drawn[0], center=True, return_mask=True)
    assert torch.equal(a[0], b[0].cpu()) and a[1].shape == b[1].shape and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) \
        and torch.equal(a[2], b[2]), "kernel path and torch specification disagree"
    h = numpy_points_in_boxes(host, drawn[0])
    assert np.array_equal(h[2], a[2].cpu().numpy()) and np.array_equal(h[1].view(np.int32), a[1].cpu().numpy().view(np.int32))
    members = int(a[0].sum())
    del a, b

    def kernel():
        return box_ops.points_in_boxes(points, next_boxes(), center=True)

    def spec():
        return box_ops.torch_points_in_boxes(points, next_boxes(), center=True)

    k_ms, s_ms = [], []
    for w in range(WARMUP + TIMED):
        state["i"] = w * CALLS
        k = host_clock(kernel, CALLS)
        state["i"] = w * CALLS
        s = host_clock(spec, CALLS)
        if w >= WARMUP:
            k_ms.append(k)
            s_ms.append(s)

    h_ms = []
    for i in range(HOST_REPEATS):
        t0 = time.perf_counter()
        numpy_points_in_boxes(host, drawn[i])
        h_ms.append((time.perf_counter() - t0) * 1e3)

    return dict(points=POINTS, columns=C, boxes=K, member_rows_first_draw=members, device=torch.cuda.get_device_name(0),
                calls_per_window=CALLS, warmup_windows=WARMUP, timed_windows=TIMED, fresh_boxes_per_call=True, launches_per_call=3,
                uploads_per_call=1, host_reads_per_call=1,
                kernel=dict(ms_per_call=round(median(k_ms), 4), min_max=[round(min(k_ms), 4), round(max(k_ms), 4)],
                            includes="planes on the host, pinned packing, 1 upload, allocations, 3 launches, host read of the counts"),
                torch=dict(ms_per_call=round(median(s_ms), 4), min_max=[round(min(s_ms), 4), round(max(s_ms), 4)]),
                kernel_not_slower=median(k_ms) <= median(s_ms), kernel_faster_than_every_torch_window=max(k_ms) < min(s_ms),
                bits_equal=True,
                host=dict(ms_per_call=round(median(h_ms), 3), min_max=[round(min(h_ms), 3), round(max(h_ms), 3)], threads=1))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("gt_database_micro.py needs a GPU: nothing is measured without one")
    path = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "gt_database_micro.json"))
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    rs = np.random.RandomState(C)
    host = ((rs.rand(POINTS, C) - 0.5) * np.array([130, 130, 10, 1, 1])).astype(np.float32)
    points = torch.from_numpy(host).to(dev)
    lines = []
    for K in BOX_COUNTS:
        lines.append(measure(dev, K, host, points))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
