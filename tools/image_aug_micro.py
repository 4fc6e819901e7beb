#!/usr/bin/env python3
"""ImageAug3D on the device: csrc/image_aug.hip (bfhip_image_aug) against the plain-torch chain, and PIL on the host.

Shape: batch 4 x 6 cameras = 24 raw uint8 frames 900 x 1600 -> [4, 6, 3, 256, 704] bf16 channels-last, normalised.  Two plans:
`train` (np.random.seed(0); resize_lim [0.38, 0.55], rot_lim [-5.4, 5.4], rand_flip: every camera its own draw, every camera
rotates) and `test` (resize 0.48, no flip, no rotation).  One JSON line per plan:

  kernel    HIP events around CALLS back-to-back calls of the C entry point (descriptors and tables prepared and uploaded
            before), median of TIMED windows after WARMUP.  Every call takes the next of SETS frame / output buffer sets whose
            total exceeds the 256 MiB Infinity Cache.  algorithmic bytes = the source bytes of each camera's crop window (the
            rows and columns its taps read) + the output; achieved bytes/s and the share of the 8 TB/s HBM peak DESIGN.md uses.
  module    Det3DDataPreprocessor.process_frames on the fused path (table packing, the upload and both allocations included)
            against the torch chain on the GPU (image_aug.torch_image_aug per sample, then process_imgs, which is the
            preprocessing kernel), alternating window by window; medians and min .. max.  `fused_faster` = the fused median is
            below the chain's minimum.  The two results are compared bit for bit first.
  fresh     (train only) what a training run sees: every call a NEW seeded draw for all 24 cameras, so every resampling table is
            new.  `fused_tables_with_plan_ms`: the tables were built with the plan (ImageAug3D(defer=True) does that, in the
            loader's worker) before the window; the consumer joins and uploads them.  `fused_tables_on_consumer_ms`: plans
            without tables and an empty coefficient cache; they are built inside the window on the thread that feeds the GPU.
            `tables_host_ms_per_batch`: wall time of building the tables of one fresh batch on one host thread (what moves to
            the worker); FRESH_TIMED windows of MODULE_CALLS calls after FRESH_WARMUP.  The `module` row above is the same
            plan call after call: its tables are built once, as in a test pipeline, never in training.
  pil       the reference's chain (resize, crop, transpose, rotate; Image.fromarray and np.array included) per frame on one
            host thread: median over the plan's six distinct cameras x PIL_REPEATS.  null when PIL is not installed.

  grid_mask_host  (with --grid-mask) the reference's GridMask of one sample on one host thread: the numpy canvas, PIL's rotate,
            the crop and the six float32 multiplies of 256 x 704 x 3; median over GRID_MASK_REPEATS draws.

--grid-mask=plain|rotated puts an active GridMask record (image_aug.GridMask(defer=True): mode 1, both axes, ratio 0.5; rotate 1
or 360) on every sample's plan: the kernel row then times bfhip_image_aug_masked with the records, the module row compares and
times both paths with the mask.  --rows=kernel,module,fresh,pil limits what is measured (default: all).

A missing GPU is an error.  Usage: image_aug_micro.py [--grid-mask=MODE] [--rows=LIST] [OUT.json]
(default OUT: profiles/image_aug_micro.json)"""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, synthetic
from bevfusion_amd import data_preprocessor as dp
from bevfusion_amd import image_aug as ia

HBM_BYTES_PER_S = 8e12
CACHE_BYTES = 256 << 20
CALLS, WARMUP, TIMED = 10, 5, 30
MODULE_CALLS = 3
PIL_REPEATS = 5
FRESH_WARMUP, FRESH_TIMED = 2, 15
GRID_MASK_REPEATS = 15
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
B, N, H, W, FINAL = 4, 6, 900, 1600, (256, 704)
TRAIN = dict(resize_lim=[0.38, 0.55], bot_pct_lim=[0.0, 0.0], rot_lim=[-5.4, 5.4], rand_flip=True, is_train=True)
TEST = dict(resize_lim=[0.48, 0.48], bot_pct_lim=[0.0, 0.0], rot_lim=[0.0, 0.0], rand_flip=False, is_train=False)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def grid_mask_cfg(mode):
    return dict(use_h=True, use_w=True, max_epoch=6, rotate=360 if mode == "rotated" else 1, ratio=0.5, mode=1, prob=1.0,
                fixed_prob=True)


def make_plans(name, seed=0, grid_mask=None):
    """Per sample (params, AugPlan): the transform's own sampler on the synthetic rig's calibration.  grid_mask ("plain" /
    "rotated"): every plan gets a drawn GridMask record (a rotated one is redrawn until its angle is not 0)."""
    rig = synthetic.camera_rig(batch=B, seed=1, train_aug=False)
    aug = ia.ImageAug3D(final_dim=FINAL, defer=True, **(TRAIN if name == "train" else TEST))
    np.random.seed(seed)
    out = []
    for b in range(B):
        data = dict(ori_shape=(H, W), cam2img=rig["camera_intrinsics"][b], cam2lidar=rig["camera2lidar"][b])
        params = [aug.sample_augmentation(data, i) for i in range(N)]
        out.append((params, ia.make_plan(params, FINAL)))
    if grid_mask:
        mask = ia.GridMask(defer=True, **grid_mask_cfg(grid_mask))
        for _, plan in out:
            mask.transform(dict(img_aug_plan=plan))
            while grid_mask == "rotated" and not plan.grid_mask[ia.GRID_MASK_COLUMNS.index("rotates")]:
                mask.transform(dict(img_aug_plan=plan))
    return out


def algorithmic_bytes(plans):
    src = 0
    for plan in plans:
        for row in np.asarray(plan):
            x0, nx, _ = ia._window(int(row[2]), FINAL[1], int(row[0]))
            y0, ny, _ = ia._window(int(row[3]), FINAL[0], int(row[1]))
            hlo, hn, _ = ia.coefficients(W, int(row[0]), x0, nx)
            vlo, vn, _ = ia.coefficients(H, int(row[1]), y0, ny)
            src += int((hlo + hn).max() - hlo.min()) * int((vlo + vn).max() - vlo.min()) * 3
    return src, B * N * 3 * FINAL[0] * FINAL[1] * 2


def kernel_row(dev, frames, plans, nbytes):
    sets = len(frames)
    n_out = B * N * 3 * FINAL[0] * FINAL[1]
    outs = [torch.empty(n_out, dtype=torch.bfloat16, device=dev) for _ in range(sets)]
    mid = torch.empty(n_out, dtype=torch.uint8, device=dev)
    prepared = [ia.descriptors(f, plans, *FINAL) for f in frames]
    tables_dev = [torch.from_numpy(t).to(dev) for _, t in prepared]
    mean, std = _lib.host_f32(MEAN), _lib.host_f32(STD)
    stream = _lib.stream_of(mid)
    state = {"k": 0}
    masks = ia.mask_records(plans)

    def call():
        k = state["k"] = (state["k"] + 1) % sets
        cams, tables = prepared[k]
        tail = (B, N, tables.ctypes.data, tables_dev[k].data_ptr(), int(tables.size), FINAL[0], FINAL[1], mid.data_ptr(), 0, 1,
                mean, std, 0.0, FINAL[0], FINAL[1], 1, 1, outs[k].data_ptr(), stream)
        if masks is None:
            _lib.call("bfhip_image_aug", cams, *tail)
        else:
            _lib.call("bfhip_image_aug_masked", cams, masks.ctypes.data, *tail)

    for _ in range(WARMUP):
        window(call, CALLS)
    ms = median([window(call, CALLS) for _ in range(TIMED)])
    rate = nbytes / (ms * 1e-3)
    return dict(kernel_ms=round(ms, 5), achieved_tb_per_s=round(rate / 1e12, 3), hbm_peak_share=round(rate / HBM_BYTES_PER_S, 3),
                table_ints=[int(t.size) for _, t in prepared][0])


def module_row(dev, frames, plans):
    sets = len(frames)
    mod = dp.Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=32, out_dtype=torch.bfloat16, channels_last=True).to(dev)
    state = {"k": 0}

    def fused():
        state["k"] = (state["k"] + 1) % sets
        return mod.process_frames(frames[state["k"]], plans)

    def chain():
        state["k"] = (state["k"] + 1) % sets
        return mod.process_imgs([ia.torch_image_aug(f, p) for f, p in zip(frames[state["k"]], plans)])

    before = dict(ia.PATHS)
    a = fused()
    state["k"] -= 1  # the chain's check runs on the same frames
    b = chain()
    assert ia.PATHS["kernel"] == before["kernel"] + 1, "the module did not take the fused path"
    assert a.shape == b.shape and a.stride() == b.stride() and torch.equal(a, b), "fused path and torch chain disagree"
    del a, b
    for _ in range(WARMUP):
        window(fused, MODULE_CALLS)
        window(chain, MODULE_CALLS)
    f_ms, c_ms = [], []
    for _ in range(TIMED):
        f_ms.append(window(fused, MODULE_CALLS))
        c_ms.append(window(chain, MODULE_CALLS))
    return dict(fused_ms=round(median(f_ms), 4), fused_ms_min_max=[round(min(f_ms), 4), round(max(f_ms), 4)],
                torch_chain_ms=round(median(c_ms), 4), torch_chain_ms_min_max=[round(min(c_ms), 4), round(max(c_ms), 4)],
                fused_faster=median(f_ms) < min(c_ms), bits_equal=True)


def fresh_row(dev, frames):
    """Training as it runs: a new draw per call."""
    sets = len(frames)
    mod = dp.Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=32, out_dtype=torch.bfloat16, channels_last=True).to(dev)
    n = (FRESH_WARMUP + FRESH_TIMED) * MODULE_CALLS
    drawn = [[p for _, p in make_plans("train", seed=100 + i)] for i in range(n)]
    build_ms = []
    for plans in drawn:  # as the loader's worker: tables with the plan
        ia._coeff_cache.clear()
        t0 = time.perf_counter()
        for p in plans:
            ia.sample_tables(p, H, W)
        build_ms.append((time.perf_counter() - t0) * 1e3)
    bare = [[ia.AugPlan(np.array(p), FINAL) for p in plans] for plans in drawn]  # the same draws without tables
    out = {}
    for key, pool in (("fused_tables_with_plan_ms", drawn), ("fused_tables_on_consumer_ms", bare)):
        state = {"k": 0, "i": 0}
        ia._coeff_cache.clear()

        def fused():
            state["k"] = (state["k"] + 1) % sets
            plans = pool[state["i"]]
            state["i"] += 1
            return mod.process_frames(frames[state["k"]], plans)

        before = ia.PATHS["kernel"]
        ms = [window(fused, MODULE_CALLS) for _ in range(FRESH_WARMUP + FRESH_TIMED)][FRESH_WARMUP:]
        assert ia.PATHS["kernel"] == before + n, "a fresh draw left the fused path"
        out[key] = round(median(ms), 4)
        out[key + "_min_max"] = [round(min(ms), 4), round(max(ms), 4)]
    out["tables_host_ms_per_batch"] = round(median(build_ms), 3)
    out["tables_host_ms_per_batch_min_max"] = [round(min(build_ms), 3), round(max(build_ms), 3)]
    out["tables_host_ms_per_frame"] = round(median(build_ms) / (B * N), 4)
    out["windows"] = [FRESH_WARMUP, FRESH_TIMED]
    return out


def pil_row(frame, params):
    try:
        from PIL import Image
    except ImportError:
        return None
    torch.set_num_threads(1)
    ms = []
    for _, dims, crop, flip, rotate in params:
        for _ in range(PIL_REPEATS):
            t0 = time.perf_counter()
            img = Image.fromarray(frame, mode="RGB").resize(dims).crop(crop)
            if flip:
                img = img.transpose(method=Image.FLIP_LEFT_RIGHT)
            np.array(img.rotate(rotate))
            ms.append((time.perf_counter() - t0) * 1e3)
    return dict(ms_per_frame=round(median(ms), 3), ms_per_frame_min_max=[round(min(ms), 3), round(max(ms), 3)],
                frames_per_s_per_core=round(1e3 / median(ms), 1), threads=1)


def grid_mask_host_row(mode):
    """The reference's GridMask.transform of one sample (six float32 frames of FINAL) restated with numpy and PIL, one thread."""
    try:
        from PIL import Image
    except ImportError:
        return None
    torch.set_num_threads(1)
    h, w = FINAL
    hh, ww = int(1.5 * h), int(1.5 * w)
    imgs = [np.random.RandomState(c).randint(0, 256, (h, w, 3)).astype(np.float32) for c in range(N)]
    mask_aug = ia.GridMask(**grid_mask_cfg(mode))
    np.random.seed(0)
    ms = []
    for _ in range(GRID_MASK_REPEATS):
        rec = dict(zip(ia.GRID_MASK_COLUMNS, mask_aug.sample(h, w).tolist()))
        t0 = time.perf_counter()
        mask = np.ones((hh, ww), np.float32)
        for i in range(hh // rec["d"]):
            s = rec["d"] * i + rec["st_h"]
            mask[s:min(s + rec["length"], hh), :] *= 0
        for i in range(ww // rec["d"]):
            s = rec["d"] * i + rec["st_w"]
            mask[:, s:min(s + rec["length"], ww)] *= 0
        mask = np.asarray(Image.fromarray(np.uint8(mask)).rotate(rec["r"]))
        mask = mask[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w].astype(np.float32)[:, :, None]
        mask = 1 - mask
        out = [x * mask for x in imgs]
        ms.append((time.perf_counter() - t0) * 1e3)
        del out
    return dict(ms_per_sample=round(median(ms), 3), ms_per_sample_min_max=[round(min(ms), 3), round(max(ms), 3)], views=N, threads=1)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("image_aug_micro.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    grid_mask = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--grid-mask=")), None)
    if grid_mask not in (None, "plain", "rotated"):
        raise SystemExit("--grid-mask=plain or --grid-mask=rotated")
    rows = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--rows=")), "kernel,module,fresh,pil").split(",")
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "image_aug_micro.json"))
    sets = CACHE_BYTES // (B * N * H * W * 3) + 2
    host = [np.ascontiguousarray(synthetic.camera_images_u8(B, N, H, W, seed=2000 + k).transpose(0, 1, 3, 4, 2)) for k in range(sets)]
    frames = [[t.contiguous() for t in torch.from_numpy(h).to(dev).unbind(0)] for h in host]
    lines = []
    for name in ("train", "test"):
        drawn = make_plans(name, grid_mask=grid_mask)
        plans = [p for _, p in drawn]
        src_bytes, out_bytes = algorithmic_bytes(plans)
        line = dict(plan=name, batch=B, views=N, source=[H, W], final_dim=list(FINAL), output="bf16 pixel-major",
                    device=torch.cuda.get_device_name(0), calls_per_window=CALLS, module_calls_per_window=MODULE_CALLS,
                    warmup_windows=WARMUP, timed_windows=TIMED, buffer_sets=sets, hbm_bytes_per_s=HBM_BYTES_PER_S,
                    resize=[round(float(p[0]), 4) for p in drawn[0][0]], rotating_cameras=int(sum(int(p[:, 5].sum()) for p in plans)),
                    algorithmic_mb=dict(crop_window_source=round(src_bytes / 1e6, 2), output=round(out_bytes / 1e6, 2)),
                    grid_mask=grid_mask, grid_mask_records=None if grid_mask is None else ia.mask_records(plans).tolist(),
                    kernel=kernel_row(dev, frames, plans, src_bytes + out_bytes) if "kernel" in rows else None,
                    module=module_row(dev, frames, plans) if "module" in rows else None,
                    fresh_draw_per_call=fresh_row(dev, frames) if name == "train" and "fresh" in rows else None,
                    pil_host=pil_row(host[0][0, 0], drawn[0][0]) if "pil" in rows else None,
                    grid_mask_host=grid_mask_host_row(grid_mask) if grid_mask and "pil" in rows else None)
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
