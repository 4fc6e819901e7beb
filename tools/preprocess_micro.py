#!/usr/bin/env python3
"""Image preprocessing: csrc/preprocess.hip (bfhip_img_preprocess) against the torch restatement of the reference's chain.

One JSON line per shape -- nuScenes (B=4, 6 views, 256 x 704) and custom_data (B=4, 5 views, 384 x 704) -- with one row per
(source dtype, output form): algorithmic bytes (input + output, from the shapes), kernel time, achieved bytes/s and the share
of the 8 TB/s HBM peak DESIGN.md uses.  Kernel time = HIP events around CALLS back-to-back calls of the C entry point into a
preallocated output, median of TIMED windows after WARMUP.  Every call takes the next of SETS input / output buffer pairs whose
total exceeds the 256 MiB Infinity Cache, so the rate is one of memory, not of a cache that holds the whole problem.

The same run times, per source dtype, the reference's chain restated in torch (data_preprocessor.torch_preprocess: per view
index, .float(), subtract, divide; per sample stack, F.pad; batch stack) followed by the .to(bf16, channels_last) pass
ResNet50.forward adds, against the module's kernel path producing the same bf16 channels-last batch (allocation included on
both sides).  The two alternate window by window; medians, and the spread (min .. max) of the chain's windows.
`kernel_not_slower` = the module's median is not above the chain's median by more than the chain's own spread (max - min).

A missing GPU is an error.  Usage: preprocess_micro.py [OUT.json]   (default OUT: profiles/preprocess_micro.json)"""
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, synthetic
from bevfusion_amd import data_preprocessor as dp

HBM_BYTES_PER_S = 8e12
CACHE_BYTES = 256 << 20
CALLS, WARMUP, TIMED = 20, 5, 30
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
SHAPES = [("nuscenes", 4, 6, 256, 704), ("custom_data", 4, 5, 384, 704)]
FORMS = [("f32", False), ("f32", True), ("bf16", False), ("bf16", True)]  # (output dtype, pixel-major)


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


def algorithmic_bytes(B, N, H, W, src, out):
    px = B * N * 3 * H * W
    return px * (1 if src == "u8" else 4) + px * (2 if out == "bf16" else 4)


_frames = {}


def sources(dev, B, N, H, W, src, sets):
    """`sets` different batches: lists of B device blocks [N, 3, H, W] of raw pixel values (seeded frames, made once)."""
    out = []
    for k in range(sets):
        key = (B, N, H, W, k)
        if key not in _frames:
            _frames[key] = torch.from_numpy(synthetic.camera_images_u8(B, N, H, W, seed=2000 + k)).to(dev)
        u8 = _frames[key]
        x = u8 if src == "u8" else u8.float() + 0.25
        out.append([t.contiguous() for t in x.unbind(0)])
    return out


def kernel_row(dev, B, N, H, W, src, form):
    out_name, pix = form
    nbytes = algorithmic_bytes(B, N, H, W, src, out_name)
    sets = CACHE_BYTES // nbytes + 2
    srcs = sources(dev, B, N, H, W, src, sets)
    dtype = torch.bfloat16 if out_name == "bf16" else torch.float32
    outs = [torch.empty((B, N, 3, H, W), dtype=dtype, device=dev) for _ in range(sets)]
    descs = [(_lib.ImgDesc * B)(*[_lib.ImgDesc(t.data_ptr(), H, W) for t in s]) for s in srcs]
    mean, std = _lib.host_f32(MEAN), _lib.host_f32(STD)
    stream = _lib.stream_of(outs[0])
    state = {"k": 0}

    def call():
        k = state["k"] = (state["k"] + 1) % sets
        _lib.call("bfhip_img_preprocess", descs[k], B, N, 0 if src == "u8" else 1, 0, 1, mean, std, 0.0, H, W,
                  1 if out_name == "bf16" else 0, int(pix), outs[k].data_ptr(), stream)

    for _ in range(WARMUP):
        window(call, CALLS)
    ms = median([window(call, CALLS) for _ in range(TIMED)])
    rate = nbytes / (ms * 1e-3)
    return dict(source=src, output=out_name + (" pixel-major" if pix else " planar"), algorithmic_mb=round(nbytes / 1e6, 2),
                buffer_sets=sets, kernel_ms=round(ms, 5), achieved_tb_per_s=round(rate / 1e12, 3),
                hbm_peak_share=round(rate / HBM_BYTES_PER_S, 3), bound="memory (bytes / 8 TB/s)")


def chain_row(dev, B, N, H, W, src):
    """Module (kernel, bf16 channels-last) against the torch chain + the backbone's cast pass, alternating windows."""
    nbytes = algorithmic_bytes(B, N, H, W, src, "bf16")
    sets = CACHE_BYTES // nbytes + 2
    srcs = sources(dev, B, N, H, W, src, sets)
    mod = dp.Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=32, out_dtype=torch.bfloat16, channels_last=True).to(dev)
    state = {"k": 0}

    def kernel():
        state["k"] = (state["k"] + 1) % sets
        return mod.process_imgs(srcs[state["k"]])

    def chain():
        state["k"] = (state["k"] + 1) % sets
        x = dp.torch_preprocess(srcs[state["k"]], mod.mean, mod.std, False, 32, 0)
        B_, N_, C_, H_, W_ = x.shape
        return x.reshape(B_ * N_, C_, H_, W_).to(dtype=torch.bfloat16, memory_format=torch.channels_last)

    before = dict(dp.LAUNCHES)
    a = kernel()
    state["k"] -= 1  # the chain's check runs on the same batch
    b = chain()
    assert dp.LAUNCHES["kernel"] == before["kernel"] + 1, "the module did not take the kernel"
    assert torch.equal(a.reshape(b.shape), b), "kernel and chain disagree"
    calls = 5
    for _ in range(WARMUP):
        window(kernel, calls)
        window(chain, calls)
    k_ms, c_ms = [], []
    for _ in range(TIMED):
        k_ms.append(window(kernel, calls))
        c_ms.append(window(chain, calls))
    return dict(source=src, output="bf16 pixel-major", module_kernel_ms=round(median(k_ms), 5),
                module_kernel_ms_min_max=[round(min(k_ms), 5), round(max(k_ms), 5)], torch_chain_ms=round(median(c_ms), 5),
                torch_chain_ms_min_max=[round(min(c_ms), 5), round(max(c_ms), 5)],
                kernel_not_slower=median(k_ms) <= median(c_ms) + (max(c_ms) - min(c_ms)), bits_equal=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_micro.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "preprocess_micro.json"))
    lines = []
    for name, B, N, H, W in SHAPES:
        line = dict(shape=name, batch=B, views=N, h=H, w=W, device=torch.cuda.get_device_name(0), calls_per_window=CALLS,
                    warmup_windows=WARMUP, timed_windows=TIMED, hbm_bytes_per_s=HBM_BYTES_PER_S,
                    kernel=[kernel_row(dev, B, N, H, W, src, form) for src in ("u8", "f32") for form in FORMS],
                    against_torch_chain=[chain_row(dev, B, N, H, W, src) for src in ("u8", "f32")])
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
