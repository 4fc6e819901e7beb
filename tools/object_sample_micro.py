#!/usr/bin/env python3
"""ObjectSample's paste on the device: the paste variant of csrc/points_aug.hip (bfhip_points_aug_paste) against the
plain-torch chain on the GPU, and the eager transforms on the host.

Shape: batch 4, POINTS = 260 000 rows per sample over +-65 m, C = 5; per sample BOXES = 40 pasted boxes (the sum of the LiDAR
config's sample_groups) of vehicle size centred on points of the cloud, and about PASTED = 3000 pasted rows inside them.  Every
call takes a FRESH draw: its own boxes and pasted rows, then BEVFusionGlobalRotScaleTrans -> BEVFusionRandomFlip3D ->
PointsRangeFilter -> PointShuffle (all deferred), made before the timed window (choosing objects, the collision test and the
file reads are the loader's work and are not measured here).  One JSON line:

  kernel    points_aug.fused_points_aug: descriptors, packing the pasted rows and plane tables into one pinned buffer, ONE
            host-to-device copy, three launches, the allocations AND the host read of the four kept counts -- the call as the
            preprocessor makes it.  A host clock around CALLS calls; median of TIMED windows after WARMUP, alternating with the
            chain window by window.
  torch     points_aug.torch_points_aug per sample on the same device tensors (the fallback path), uploads included.
  host      the eager point work per sample on ONE host thread: the paste (box test, gather, concatenate) and then the eager
            chain; `paste_ms` is the paste alone.  Median over HOST_REPEATS samples.

The kernel's and the chain's outputs are compared bit for bit first.  A missing GPU is an error.
Usage: object_sample_micro.py [OUT.json]   (default OUT: profiles/object_sample_micro.json)"""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import points_aug as pa

B, POINTS, C, BOXES, PASTED = 4, 260000, 5, 40, 3000
RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
GRST = dict(rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5])
CALLS, WARMUP, TIMED = 5, 3, 20
HOST_REPEATS = 5


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def chain(defer):
    return [pa.BEVFusionGlobalRotScaleTrans(defer=defer, **GRST), pa.BEVFusionRandomFlip3D(defer=defer),
            pa.PointsRangeFilter(RANGE, defer=defer), pa.PointShuffle(defer=defer)]


def draw_paste(rs, cloud):
    """(pasted rows [about PASTED, C], boxes [BOXES, 7]): vehicle-sized boxes on points of the cloud, rows inside them."""
    at = cloud[rs.randint(0, len(cloud), BOXES), :3]
    boxes = np.concatenate([at - np.array([0, 0, 0.8]), rs.uniform([3.5, 1.6, 1.4], [11.0, 2.9, 3.5], (BOXES, 3)),
                            rs.uniform(-np.pi, np.pi, (BOXES, 1))], 1).astype(np.float32)
    per = rs.randint(PASTED // BOXES // 2, PASTED // BOXES * 3 // 2 + 1, BOXES)
    rows = []
    for b, n in zip(boxes, per):
        local = (rs.rand(n, C) - 0.5) * np.array([b[3], b[4], b[5], 1, 1])
        c, s = np.cos(b[6]), np.sin(b[6])
        xy = local[:, :2] @ np.array([[c, s], [-s, c]])
        rows.append(np.concatenate([xy + b[:2], local[:, 2:3] + b[2] + b[5] / 2, local[:, 3:] + 0.5], 1))
    return np.concatenate(rows, 0).astype(np.float32), boxes


def draw_plans(seed, host):
    """The deferred pipeline's plans of one batch under one seed."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    plans = []
    stand_in = torch.zeros((1, 3))  # deferred transforms never look at the points
    for i in range(B):
        data = dict(points=stand_in)
        pa._plan_of(data).set_paste(*draw_paste(rs, host[i]))
        for t in chain(True):
            data = t.transform(data)
        plans.append(data["points_aug_plan"])
    return plans


def host_clock(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def measure(dev):
    rs = np.random.RandomState(C)
    host = [((rs.rand(POINTS, C) - 0.5) * np.array([130, 130, 10, 1, 1][:C])).astype(np.float32) for _ in range(B)]
    points = [torch.from_numpy(h).to(dev) for h in host]
    n_draws = (WARMUP + TIMED) * CALLS
    drawn = [draw_plans(1000 + i, host) for i in range(n_draws)]
    state = {"i": 0}

    def next_plans():
        plans = drawn[state["i"] % n_draws]
        state["i"] += 1
        return plans

    assert pa.fused_supported(points, drawn[0])
    a = pa.fused_points_aug(points, drawn[0])
    b = [pa.torch_points_aug(p, plan) for p, plan in zip(points, drawn[0])]
    assert all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), \
        "kernel path and torch chain disagree"
    kept = [int(x.shape[0]) for x in a]
    removed = [int(pa.points_in_any_box(p, torch.from_numpy(plan.paste_planes).to(dev)).sum()) for p, plan in zip(points, drawn[0])]
    pasted = [int(plan.paste_points.shape[0]) for plan in drawn[0]]
    del a, b

    def fused():
        return pa.fused_points_aug(points, next_plans())

    def torch_chain():
        return [pa.torch_points_aug(p, plan) for p, plan in zip(points, next_plans())]

    f_ms, c_ms = [], []
    for w in range(WARMUP + TIMED):
        state["i"] = w * CALLS
        f = host_clock(fused, CALLS)
        state["i"] = w * CALLS
        c = host_clock(torch_chain, CALLS)
        if w >= WARMUP:
            f_ms.append(f)
            c_ms.append(c)

    torch.set_num_threads(1)
    h_ms, p_ms = [], []
    for i in range(HOST_REPEATS):
        np.random.seed(2000 + i)
        torch.manual_seed(2000 + i)
        data = dict(points=torch.from_numpy(host[i % B].copy()))
        paste = pa.PointsAugPlan()  # the paste of a drawn plan alone: what ObjectSample(defer=False) applies
        paste.paste_points, paste.paste_planes = drawn[i][i % B].paste_points, drawn[i][i % B].paste_planes
        t0 = time.perf_counter()
        pa._apply(data, paste)
        t1 = time.perf_counter()
        for t in chain(False):
            data = t.transform(data)
        h_ms.append((time.perf_counter() - t0) * 1e3)
        p_ms.append((t1 - t0) * 1e3)

    return dict(batch=B, points_per_sample=POINTS, columns=C, boxes_per_sample=BOXES, pasted_rows_first_draw=pasted,
                removed_first_draw=removed, kept_first_draw=kept, device=torch.cuda.get_device_name(0), calls_per_window=CALLS,
                warmup_windows=WARMUP, timed_windows=TIMED, fresh_draw_per_call=True, launches_per_batch=3,
                uploads_per_batch=1, host_reads_per_batch=1,
                kernel=dict(ms_per_batch=round(median(f_ms), 4), min_max=[round(min(f_ms), 4), round(max(f_ms), 4)],
                            includes="descriptors, pinned packing, 1 upload, allocations, 3 launches, host read of the kept counts"),
                torch=dict(ms_per_batch=round(median(c_ms), 4), min_max=[round(min(c_ms), 4), round(max(c_ms), 4)]),
                kernel_faster=median(f_ms) < min(c_ms), bits_equal=True,
                host=dict(ms_per_sample=round(median(h_ms), 3), min_max=[round(min(h_ms), 3), round(max(h_ms), 3)],
                          paste_ms_per_sample=round(median(p_ms), 3), ms_per_batch=round(median(h_ms) * B, 3), threads=1))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("object_sample_micro.py needs a GPU: nothing is measured without one")
    path = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "object_sample_micro.json"))
    line = measure(torch.device("cuda:0"))
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump([line], f, indent=1)
        f.write("\n")
