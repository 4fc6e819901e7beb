#!/usr/bin/env python3
"""Query initialisation of the TransFusion head: csrc/query_init.hip (query_init.fused_query_init) against the torch chain of
BEVFusionHead.forward (max_pool2d, mask, topk, //, %, indexing gather, bev_pos gather, score gather), forward alone and
forward + backward of the rows, in one process.

Shapes: the nuScenes head at batch 4 (C=10, 180 x 180, K=200, 128 bf16 channels) and the custom_data head (C=5, K=500).  The
score map is sigmoid(N(-2.19, 1)) per cell, in both memory layouts; about one interior cell in nine is a 3x3 peak (~35 000
candidates a sample at C=10: more than a trained head's smooth map has).  The two arms ALTERNATE: PAIRS times (fused window, torch
window), a window = CALLS back-to-back calls between HIP events; reported per call as the median over the windows, with
the host time to issue a call (a host clock around the window's enqueue loop, before the synchronise) beside the device time.
One JSON line per (shape, layout, pass).  A missing GPU is an error.

Usage: query_init_micro.py [OUT.json]   (default OUT: profiles/query_init_micro.json)"""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

import bevfusion_amd  # noqa: F401
from bevfusion_amd import query_init as qi

CALLS, WARMUP, PAIRS = 10, 3, 15
# (name, B, C, H, W, K, Ch)
SHAPES = [("nuscenes batch 4", 4, 10, 180, 180, 200, 128), ("custom_data batch 4", 4, 5, 180, 180, 500, 128),
          ("nuscenes batch 1", 1, 10, 180, 180, 200, 128)]


def torch_chain(h, flat, K, bev_pos):
    B, C = h.shape[:2]
    local_max = torch.zeros_like(h)
    inner = F.max_pool2d(h, kernel_size=3, stride=1, padding=0)
    local_max[:, :, 1:-1, 1:-1] = inner
    heatmap = (h * (h == local_max)).reshape(B, C, -1)
    top = heatmap.reshape(B, -1).topk(K, dim=-1).indices
    top_class, top_index = top // heatmap.shape[-1], top % heatmap.shape[-1]
    rows = flat.transpose(1, 2)[torch.arange(B, device=flat.device)[:, None], top_index]
    one_hot = F.one_hot(top_class, num_classes=C)   # the chain's consumer of top_class (kept in both arms)
    query_pos = bev_pos.expand(B, -1, -1).gather(index=top_index[:, :, None].expand(-1, -1, 2), dim=1)
    score = heatmap.gather(index=top_index[:, None, :].expand(-1, C, -1), dim=-1)
    return top_class, top_index, query_pos, score, rows, one_hot


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    host = (time.perf_counter() - t0) / CALLS
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS, host * 1e3


def measure(dev, name, B, C, H, W, K, Ch, layout, backward):
    g = torch.Generator().manual_seed(0)
    h = torch.sigmoid(torch.randn(B, C, H, W, generator=g) - 2.19).to(dev)
    if layout == "nhwc":
        h = h.contiguous(memory_format=torch.channels_last)
    feat = torch.randn(B, H * W, Ch, generator=g).to(dev, torch.bfloat16)
    d_rows = torch.randn(B, K, Ch, generator=g).to(dev, torch.bfloat16)
    bx, by = torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), indexing="ij")
    bev_pos = torch.stack([bx + 0.5, by + 0.5], 0).view(1, 2, -1).permute(0, 2, 1).to(dev)
    assert qi.supported(h, feat.transpose(1, 2), K)

    def arm(fused):
        def run():
            flat = feat.transpose(1, 2)
            if backward:
                flat = flat.detach().requires_grad_(True)
            if fused:
                out = qi.fused_query_init(h, flat, K, W)
                F.one_hot(out[0], num_classes=C)
            else:
                out = torch_chain(h, flat, K, bev_pos)
            if backward:
                out[4].backward(d_rows)
            return out
        return run

    fused, chain = arm(True), arm(False)
    a, b = fused(), chain()
    same = all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))   # ties between random scores are possible: reported, not assumed
    for _ in range(WARMUP):
        window(fused)
        window(chain)
    res = dict(fused=[], torch=[])
    for _ in range(PAIRS):
        res["fused"].append(window(fused))
        res["torch"].append(window(chain))
    row = dict(shape=name, B=B, C=C, H=H, W=W, K=K, Ch=Ch, layout=layout, backward=backward, outputs_equal=same,
               calls_per_window=CALLS, pairs=PAIRS)
    for k, v in res.items():
        row[k + "_device_ms"] = round(median([x[0] for x in v]), 5)
        row[k + "_device_ms_min_max"] = [round(min(x[0] for x in v), 5), round(max(x[0] for x in v), 5)]
        row[k + "_host_issue_ms"] = round(median([x[1] for x in v]), 5)
    row["fused_faster"] = row["fused_device_ms"] < row["torch_device_ms"]
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("query_init_micro.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "query_init_micro.json"))
    rows = [measure(dev, *shape, layout, backward) for shape in SHAPES for layout in ("nhwc", "nchw") for backward in (False, True)]
    with open(out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)
        f.write("\n")
