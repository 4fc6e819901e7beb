#!/usr/bin/env python3
"""Eval-mode BatchNorm (+ residual) (+ ReLU): csrc/bn_eval.hip (bn2d.FUSED_BN_EVAL on) against the torch path (off).

1. Per-op table: activations of a batch-4 step of the default nuScenes model (24 camera images of 256 x 704) in bf16 -- the
   ResNet-50 stem norm and the bottlenecks' bn1 / bn3 per stage, SECOND's two stages, a depthnet layer -- with and without a
   residual, ReLU on.  Both arms are the same `BatchNorm2dAct` in eval() under no_grad; only the switch differs.  HIP events
   around CALLS back-to-back calls, 5 warm-up + 30 timed windows, median, reported per call.  HBM fraction = algorithmic bytes
   (2 + residual) * M * C * sizeof(bf16) over 8 TB/s, over the measured time.
2. Whole model: `BEVFusion.predict` of nuscenes_config() (ResNet-50, camera + LiDAR) on synthetic inputs in eval() under no_grad
   and bf16 autocast at batch 1 and batch 4; three runs with the switch on and three with it off, alternating in one process
   (a run = median of --predict-steps calls between HIP events).  `ships_on` is the rule of DESIGN.md section 6: every run with
   the switch on below every run with it off, at both batch sizes.

A missing GPU is an error.  Usage: bn_eval_micro.py [OUT.json] [--skip-model] [--predict-steps 5]
(default OUT: profiles/bn_eval_micro.json)"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import bn2d, synthetic
from bevfusion_amd.bevfusion import nuscenes_config
from bevfusion_amd.registry import MODELS

HBM_BYTES_PER_S = 8e12
CALLS, WARMUP, TIMED = 10, 5, 30

# (name, N, C, H, W): batch 4 = 24 camera images of 256 x 704; BEV grid 180 x 180
LAYERS = [
    ("resnet50 stem bn1", 24, 64, 128, 352),
    ("resnet50 layer1 bn1", 24, 64, 64, 176),
    ("resnet50 layer1 bn3", 24, 256, 64, 176),
    ("resnet50 layer2 bn3", 24, 512, 32, 88),
    ("resnet50 layer3 bn3", 24, 1024, 16, 44),
    ("resnet50 layer4 bn3", 24, 2048, 8, 22),
    ("SECOND stage 1", 4, 128, 180, 180),
    ("SECOND stage 2", 4, 256, 90, 90),
    ("depthnet 256 ch", 24, 256, 32, 88),
]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def time_calls(fn):
    for _ in range(WARMUP):
        for _ in range(CALLS):
            fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / CALLS)
    return median(ms)


def op_table(dev):
    rows = []
    for name, N, C, H, W in LAYERS:
        torch.manual_seed(0)
        x = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        r = torch.randn(N, C, H, W, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        bn = bn2d.BatchNorm2dAct(C, eps=1e-5).to(dev).eval()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
            for res in (None, r):
                row = dict(layer=name, shape=[N, C, H, W], residual=res is not None)
                for arm, flag in (("hip_ms", True), ("torch_ms", False)):
                    bn2d.FUSED_BN_EVAL = flag
                    before = bn2d.EVAL_LAUNCHES["fwd"]
                    row[arm] = round(time_calls(lambda: bn(x, residual=res, relu=True)), 5)
                    assert (bn2d.EVAL_LAUNCHES["fwd"] > before) == flag, "the switch did not select the arm"
                nbytes = (2 + (res is not None)) * x.numel() * 2
                row["algorithmic_mb"] = round(nbytes / 1e6, 2)
                row["hip_hbm_fraction"] = round(nbytes / HBM_BYTES_PER_S / (row["hip_ms"] * 1e-3), 3)
                row["torch_hbm_fraction"] = round(nbytes / HBM_BYTES_PER_S / (row["torch_ms"] * 1e-3), 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def predict_inputs(dev, B):
    d = {"points": [torch.from_numpy(synthetic.lidar_sweep(40000, seed=1000 + i)).to(dev) for i in range(B)]}
    rig = synthetic.camera_rig(batch=B, seed=1, train_aug=False)
    d["imgs"] = torch.randn(B, 6, 3, 256, 704, device=dev)
    for src, dst in (("lidar2image", "lidar2img"), ("camera_intrinsics", "cam2img"), ("camera2lidar", "cam2lidar"),
                     ("img_aug_matrix", "img_aug_matrix"), ("lidar_aug_matrix", "lidar_aug_matrix")):
        d[dst] = torch.from_numpy(rig[src]).to(dev)
    return d


def predict_pairs(dev, steps):
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config()).to(dev).eval()
    out = []
    for B in (1, 4):
        inp = predict_inputs(dev, B)

        def run(flag, n):
            bn2d.FUSED_BN_EVAL = flag
            before = bn2d.EVAL_LAUNCHES["fwd"]
            ms = []
            for _ in range(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    model.predict(inp)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            return median(ms), (bn2d.EVAL_LAUNCHES["fwd"] - before) // n

        for flag in (True, False, True, False):  # warm-up of both arms
            run(flag, 1)
        res = dict(batch=B, steps_per_run=steps, on_ms=[], off_ms=[])
        for _ in range(3):
            for flag in (True, False):
                ms, launches = run(flag, steps)
                res["on_ms" if flag else "off_ms"].append(round(ms, 3))
                if flag:
                    res["eval_bn_kernel_calls_per_predict"] = launches
                else:
                    assert launches == 0
        res["every_on_below_every_off"] = max(res["on_ms"]) < min(res["off_ms"])
        out.append(res)
        print(json.dumps(res), flush=True)
    return out


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("bn_eval_micro.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "bn_eval_micro.json"))
    shipped = bn2d.FUSED_BN_EVAL
    res = dict(device=torch.cuda.get_device_name(0), dtype="bf16", relu=True, calls_per_window=CALLS, warmup_windows=WARMUP,
               timed_windows=TIMED, hbm_bytes_per_s=HBM_BYTES_PER_S, ops=op_table(dev))

    def write():
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    write()  # the per-op table survives a failure of the model part
    if "--skip-model" not in sys.argv:
        res["predict"] = predict_pairs(dev, int(arg("--predict-steps", 5)))
        res["ships_on"] = all(p["every_on_below_every_off"] for p in res["predict"])
        write()
    bn2d.FUSED_BN_EVAL = shipped
