#!/usr/bin/env python3
"""LoadPointsFromMultiSweeps on the device: the sweep variants of csrc/points_aug.hip (bfhip_points_aug_sweeps) against the
plain-torch chain on the GPU, and the eager transforms on the host.

Shape: batch 4; per sample a keyframe of KEY = 26 000 rows and SWEEPS = 9 sweeps of about 26 000 rows (C = 5, returns over
+-60 m, 2 % of every cloud inside the 1 m square), rigid float64 lidar2sensor matrices; BOXES = 40 pasted boxes with about
PASTED = 3000 pasted rows; then BEVFusionGlobalRotScaleTrans -> BEVFusionRandomFlip3D -> PointsRangeFilter -> PointShuffle.
Every call takes a FRESH draw of the paste and the chain (made before the timed window); the clouds are the same raw buffers,
one per sample, in pinned host memory as a loader's collate would leave them.  One JSON line:

  kernel    the upload of the four raw buffers (one copy each) and points_aug.fused_points_aug: descriptors, packing the segment
            tables, pasted rows and plane tables into one pinned buffer, ONE host-to-device copy, three launches, the allocations
            AND the host read of the four kept counts.  A host clock around CALLS calls; median of TIMED windows after WARMUP,
            alternating with the chain window by window.
  torch     the same uploads and points_aug.torch_points_aug per sample on the device (the fallback path).
  host      the eager point work per sample on ONE host thread, from the clouds in memory (no file reads): the sweep step, the
            paste and the eager chain; `sweeps_ms` is the sweep step alone.  Median over HOST_REPEATS samples.

The kernel's and the chain's outputs are compared bit for bit first.  A missing GPU is an error.
Usage: multi_sweep_micro.py [OUT.json]   (default OUT: profiles/multi_sweep_micro.json)"""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import points_aug as pa
from bevfusion_amd import synthetic
from object_sample_micro import chain, draw_paste, host_clock, median

B, KEY, SWEEPS, C = 4, 26000, 9, 5
CALLS, WARMUP, TIMED = 5, 3, 20
HOST_REPEATS = 5


def make_samples():
    """Per sample (the raw buffer [keyframe ; sweeps] float32 [n, C], starts, lidar2sensor, dt)."""
    out = []
    for i in range(B):
        s = synthetic.multi_sweep_sample(seed=4000 + i, key_rows=KEY, sweep_rows=KEY, sweeps=SWEEPS, features=C)
        clouds = [s["keyframe"]] + s["sweeps"]
        starts = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
        out.append((np.concatenate(clouds, 0), starts, s["lidar2sensor"], np.float32(s["timestamp"] - s["sweep_timestamps"])))
    return out


def draw_plans(seed, samples):
    """The deferred pipeline's plans of one batch under one seed: the sweep step, a paste, the chain."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    plans = []
    stand_in = torch.zeros((1, 3))  # deferred transforms never look at the points
    for rows, starts, l2s, dt in samples:
        data = dict(points=stand_in)
        pa._plan_of(data).set_sweeps(starts, l2s, dt, True).set_paste(*draw_paste(rs, rows[:KEY]))
        for t in chain(True):
            data = t.transform(data)
        plans.append(data["points_aug_plan"])
    return plans


def measure(dev):
    samples = make_samples()
    pinned = [torch.from_numpy(rows).pin_memory() for rows, _, _, _ in samples]
    n_draws = (WARMUP + TIMED) * CALLS
    drawn = [draw_plans(1000 + i, samples) for i in range(n_draws)]
    state = {"i": 0}

    def next_plans():
        plans = drawn[state["i"] % n_draws]
        state["i"] += 1
        return plans

    def upload():
        return [p.to(dev, non_blocking=True) for p in pinned]

    points = upload()
    assert pa.fused_supported(points, drawn[0])
    a = pa.fused_points_aug(points, drawn[0])
    b = [pa.torch_points_aug(p, plan) for p, plan in zip(points, drawn[0])]
    assert all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), \
        "kernel path and torch chain disagree"
    kept = [int(x.shape[0]) for x in a]
    swept = [int(pa.sweep_rows(p, plan).shape[0]) for p, plan in zip(points, drawn[0])]
    rows = [int(p.shape[0]) for p in points]
    del a, b, points

    def fused():
        return pa.fused_points_aug(upload(), next_plans())

    def torch_chain():
        return [pa.torch_points_aug(p, plan) for p, plan in zip(upload(), next_plans())]

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
    h_ms, s_ms = [], []
    for i in range(HOST_REPEATS):
        np.random.seed(2000 + i)
        torch.manual_seed(2000 + i)
        raw, plan = samples[i % B][0], drawn[i][i % B]
        data = dict(points=torch.from_numpy(raw.copy()))
        sweeps, paste = pa.PointsAugPlan(), pa.PointsAugPlan()  # the two first steps as the eager transforms apply them
        for k in pa.PointsAugPlan._SWEEPS:
            setattr(sweeps, k, getattr(plan, k))
        paste.paste_points, paste.paste_planes = plan.paste_points, plan.paste_planes
        t0 = time.perf_counter()
        pa._apply(data, sweeps)
        t1 = time.perf_counter()
        pa._apply(data, paste)
        for t in chain(False):
            data = t.transform(data)
        h_ms.append((time.perf_counter() - t0) * 1e3)
        s_ms.append((t1 - t0) * 1e3)

    return dict(batch=B, rows_per_sample=rows, sweeps_per_sample=SWEEPS, columns=C, rows_after_remove_close_first_draw=swept,
                kept_first_draw=kept, device=torch.cuda.get_device_name(0), calls_per_window=CALLS, warmup_windows=WARMUP,
                timed_windows=TIMED, fresh_draw_per_call=True, launches_per_batch=3, table_uploads_per_batch=1,
                host_reads_per_batch=1,
                kernel=dict(ms_per_batch=round(median(f_ms), 4), min_max=[round(min(f_ms), 4), round(max(f_ms), 4)],
                            includes="upload of the raw buffers, descriptors, pinned packing, 1 table upload, allocations, "
                                     "3 launches, host read of the kept counts"),
                torch=dict(ms_per_batch=round(median(c_ms), 4), min_max=[round(min(c_ms), 4), round(max(c_ms), 4)],
                           includes="upload of the raw buffers, torch_points_aug per sample"),
                kernel_faster=median(f_ms) < min(c_ms), bits_equal=True,
                host=dict(ms_per_sample=round(median(h_ms), 3), min_max=[round(min(h_ms), 3), round(max(h_ms), 3)],
                          sweeps_ms_per_sample=round(median(s_ms), 3), ms_per_batch=round(median(h_ms) * B, 3), threads=1))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("multi_sweep_micro.py needs a GPU: nothing is measured without one")
    path = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "multi_sweep_micro.json"))
    line = measure(torch.device("cuda:0"))
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump([line], f, indent=1)
        f.write("\n")
