#!/usr/bin/env python3
"""The deferred LiDAR augmentation on the device: csrc/points_aug.hip (bfhip_points_aug) against the plain-torch chain on the
GPU, and the eager transforms on the host.

Shape: batch 4, POINTS = 260 000 rows per sample over +-65 m (about half leave the +-54 m range), C = 5 (nuScenes: x, y, z,
intensity, dt) and C = 3 (the custom_data shape).  Every call takes a FRESH draw: the chain BEVFusionGlobalRotScaleTrans ->
BEVFusionRandomFlip3D -> PointsRangeFilter -> PointShuffle (all deferred) under its own seed, sampled before the timed window
(that is the loader's work).  One JSON line per shape:

  kernel    points_aug.fused_points_aug: descriptors, three launches (count, scan, ranked write), the output, count and
            workspace allocations AND the host read of the four kept counts -- the call as the preprocessor makes it.  A host
            clock around CALLS calls, each of which ends in that read (a device-to-host copy that waits for the launches); median
            of TIMED windows after WARMUP, alternating with the chain window by window.
  torch     points_aug.torch_points_aug per sample on the same device tensors (the fallback path; its boolean indexing and the
            cycle walk's `any()` read the device too).
  launch_only  HIP events around CALLS calls of the C entry point alone (descriptors and buffers prepared, no host read):
            what the three launches cost.  algorithmic bytes = n * C * 4 read twice (count and write pass) + kept * C * 4 written.
            The same 21 MB (C = 5) of points are read on every call, so they stay in the 256 MiB Infinity Cache: the rate is
            what the launches achieve on cache-resident data, not an HBM figure; `hbm_peak_share` only sets it beside 8 TB/s.
  host      the eager chain (defer=False) per sample on ONE host thread: median over HOST_REPEATS samples.

The kernel's and the chain's outputs are compared bit for bit first.  A missing GPU is an error.
Usage: points_aug_micro.py [OUT.json]   (default OUT: profiles/points_aug_micro.json)"""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib
from bevfusion_amd import points_aug as pa

HBM_BYTES_PER_S = 8e12
B, POINTS = 4, 260000
RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
GRST = dict(rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5])
CALLS, WARMUP, TIMED = 5, 3, 20
HOST_REPEATS = 5
LAUNCHES_PER_BATCH = 3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def chain(defer):
    return [pa.BEVFusionGlobalRotScaleTrans(defer=defer, **GRST), pa.BEVFusionRandomFlip3D(defer=defer),
            pa.PointsRangeFilter(RANGE, defer=defer), pa.PointShuffle(defer=defer)]


def draw_plans(seed):
    """The deferred chain's plans of one batch under one seed."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    plans = []
    stand_in = torch.zeros((1, 3))  # deferred transforms never look at the points
    for _ in range(B):
        data = dict(points=stand_in)
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


def event_clock(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def shape_row(dev, C):
    rs = np.random.RandomState(C)
    host = [((rs.rand(POINTS, C) - 0.5) * np.array([130, 130, 10, 1, 1][:C])).astype(np.float32) for _ in range(B)]
    points = [torch.from_numpy(h).to(dev) for h in host]
    n_draws = (WARMUP + TIMED) * CALLS
    drawn = [draw_plans(1000 + i) for i in range(n_draws)]
    state = {"i": 0}

    def next_plans():
        plans = drawn[state["i"] % n_draws]
        state["i"] += 1
        return plans

    a = pa.fused_points_aug(points, drawn[0])
    b = [pa.torch_points_aug(p, plan) for p, plan in zip(points, drawn[0])]
    assert all(x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), \
        "kernel path and torch chain disagree"
    kept = [int(x.shape[0]) for x in a]
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

    # the launches alone
    total = B * POINTS
    out = torch.empty((total, C), dtype=torch.float32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = _lib.call_size("bfhip_points_aug_workspace_bytes", total, B)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    prepared = [pa.descriptors(points, plans) for plans in drawn[:CALLS]]
    stream = _lib.stream_of(out)
    k = {"i": 0}

    def launches():
        k["i"] = (k["i"] + 1) % len(prepared)
        _lib.call("bfhip_points_aug", prepared[k["i"]], B, C, out.data_ptr(), counts.data_ptr(), work.data_ptr(), nbytes, stream)

    for _ in range(WARMUP):
        event_clock(launches, CALLS)
    l_ms = [event_clock(launches, CALLS) for _ in range(TIMED)]
    alg = 2 * total * C * 4 + sum(kept) * C * 4
    rate = alg / (median(l_ms) * 1e-3)

    torch.set_num_threads(1)
    h_ms = []
    for i in range(HOST_REPEATS):
        np.random.seed(2000 + i)
        torch.manual_seed(2000 + i)
        data = dict(points=torch.from_numpy(host[i % B].copy()))
        t0 = time.perf_counter()
        for t in chain(False):
            data = t.transform(data)
        h_ms.append((time.perf_counter() - t0) * 1e3)

    return dict(batch=B, points_per_sample=POINTS, columns=C, kept_first_draw=kept, device=torch.cuda.get_device_name(0),
                calls_per_window=CALLS, warmup_windows=WARMUP, timed_windows=TIMED, fresh_draw_per_call=True,
                launches_per_batch=LAUNCHES_PER_BATCH, host_reads_per_batch=1,
                kernel=dict(ms_per_batch=round(median(f_ms), 4), min_max=[round(min(f_ms), 4), round(max(f_ms), 4)],
                            includes="descriptors, allocations, 3 launches, host read of the kept counts"),
                torch=dict(ms_per_batch=round(median(c_ms), 4), min_max=[round(min(c_ms), 4), round(max(c_ms), 4)]),
                kernel_faster=median(f_ms) < min(c_ms), bits_equal=True,
                launch_only=dict(ms_per_batch=round(median(l_ms), 5), min_max=[round(min(l_ms), 5), round(max(l_ms), 5)],
                                 algorithmic_mb=round(alg / 1e6, 2), achieved_tb_per_s=round(rate / 1e12, 3),
                                 hbm_peak_share=round(rate / HBM_BYTES_PER_S, 3)),
                host=dict(ms_per_sample=round(median(h_ms), 3), min_max=[round(min(h_ms), 3), round(max(h_ms), 3)],
                          ms_per_batch=round(median(h_ms) * B, 3), threads=1))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("points_aug_micro.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    path = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "points_aug_micro.json"))
    lines = []
    for C in (5, 3):
        line = shape_row(dev, C)
        lines.append(line)
        print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
