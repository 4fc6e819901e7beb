#!/usr/bin/env python3
"""Training-step time of the custom_data model (bevfusion.custom_data_config: five 384 x 704 cameras, Swin-T, three point
features, 500 proposals, 5 classes) at batch 1 and batch 4: forward + real loss + backward + clip + AdamW under bf16
autocast on synthetic inputs, LiDAR branch on the side stream, timed eagerly between HIP events.  A number for later
rounds, no target.  Usage: custom_step.py [OUT.json] [--batches 1,4] [--steps 5] [--warmup 3]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import attention, synthetic
from bevfusion_amd.amp import MasterWeightAdamW
from bevfusion_amd.bevfusion import custom_data_config
from bevfusion_amd.registry import MODELS


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def run(dev, B, steps, warmup):
    C = synthetic.CUSTOM
    torch.manual_seed(0)
    model = MODELS.build(custom_data_config()).to(dev).train()
    model.lidar_side_stream = True
    model.view_transform.conv_dtype = torch.bfloat16
    opt = MasterWeightAdamW(model, lr=2e-4, weight_decay=0.01, max_grad_norm=35.0)
    rig = synthetic.camera_rig(batch=B, seed=1, train_aug=True, **C["rig"])
    inp = {"points": [torch.from_numpy(synthetic.lidar_sweep(40000, seed=1000 + i, features=C["point_features"])).to(dev)
                      for i in range(B)],
           "imgs": torch.randn(B, C["num_cams"], 3, *C["image_size"], device=dev)}
    for src, dst in (("lidar2image", "lidar2img"), ("camera_intrinsics", "cam2img"), ("camera2lidar", "cam2lidar"),
                     ("img_aug_matrix", "img_aug_matrix"), ("lidar_aug_matrix", "lidar_aug_matrix")):
        inp[dst] = torch.from_numpy(rig[src]).to(dev)
    gts = [tuple(torch.from_numpy(a) for a in synthetic.gt_boxes(seed=3000 + i, classes=C["classes"])) for i in range(B)]

    def step():
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            total, _ = model.parse_losses(model.loss(inp, gts))
        total.backward()
        opt.step()
        return total

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        loss = step()
        b.record()
        torch.cuda.synchronize()
        times.append((a.elapsed_time(b), (time.perf_counter() - t0) * 1e3))
    assert torch.isfinite(loss)
    gpu = sorted(t[0] for t in times)
    return dict(batch=B, steps=steps, warmup=warmup, step_ms_median=round(gpu[len(gpu) // 2], 3), step_ms_min=round(gpu[0], 3),
                wall_ms_median=round(sorted(t[1] for t in times)[len(times) // 2], 3), loss=float(loss.detach()),
                peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), None)
    res = dict(model="custom_data_config() camera + LiDAR, bf16 autocast, 40k points / sample", device=torch.cuda.get_device_name(0),
               wide_attention_kernel=attention.WIDE, runs=[])
    for B in [int(b) for b in arg("--batches", "1,4").split(",")]:
        torch.cuda.reset_peak_memory_stats()
        res["runs"].append(run(dev, B, int(arg("--steps", 5)), int(arg("--warmup", 3))))
        print(json.dumps(res["runs"][-1]), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
