#!/usr/bin/env python3
"""JPEG decode split at the entropy stage: the host half against Pillow, and the device half (csrc/jpeg.hip) on the GPU.

Batch: 24 frames (4 samples x 6 cameras) of the fixture frame tests/golden/nus_cam_front.jpg, 1600 x 900, 4:2:0.  One JSON object:

  host      one thread: milliseconds per frame of Pillow's whole decode (Image.open(...).convert("RGB") into a numpy array;
            null when PIL is not installed) and of bfhip_jpeg_entropy_decode (parse included) on the same bytes; median and
            min .. max over HOST_REPEATS.
  device    HIP events around CALLS back-to-back calls of bfhip_jpeg_decode (both launches; coefficients and descriptor
            table uploaded before), median of TIMED windows after WARMUP.  Every call takes the next of SETS coefficient /
            plane / output buffer sets whose total exceeds the 256 MiB Infinity Cache.  algorithmic bytes = coefficients in +
            planes written and read back + RGB out; achieved bytes/s and the share of the 8 TB/s HBM peak DESIGN.md uses.
  upload    the coefficient bytes of one frame against its decoded bytes.
  bits      the batch's first frame from the device equals jpeg.torch_jpeg_decode, checked before timing.

A missing GPU is an error.  Usage: jpeg_micro.py [--rows=host,device] [OUT.json]  (default OUT: profiles/jpeg_micro.json)"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, jpeg

HBM_BYTES_PER_S = 8e12
CACHE_BYTES = 256 << 20
FRAMES = 24
CALLS, WARMUP, TIMED = 10, 5, 30
HOST_REPEATS = 15
FIXTURE = os.path.join(ROOT, "tests", "golden", "nus_cam_front.jpg")


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def host_row(data):
    torch.set_num_threads(1)
    arr = np.frombuffer(data, np.uint8)

    def timed(fn):
        fn()
        ms = []
        for _ in range(HOST_REPEATS):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return dict(ms_per_frame=round(median(ms), 3), ms_per_frame_min_max=[round(min(ms), 3), round(max(ms), 3)])

    header = jpeg.parse(arr)
    coef = np.empty(header.coef_bytes // 2, np.int16)
    row = dict(threads=1, entropy_stage=timed(lambda: jpeg.entropy_decode(arr, jpeg.parse(arr), coef)))
    try:
        import io
        from PIL import Image
        row["pillow_full_decode"] = timed(lambda: np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
        row["entropy_over_pillow"] = round(row["entropy_stage"]["ms_per_frame"] / row["pillow_full_decode"]["ms_per_frame"], 3)
    except ImportError:
        row["pillow_full_decode"] = None
    return row


def device_row(dev, header, coef):
    frames = [(header, coef)] * FRAMES
    planes_bytes = sum(header.block_cols[c] * header.block_rows[c] * 64 for c in range(3)) * FRAMES
    rgb_bytes = header.width * header.height * 3 * FRAMES
    per_set = header.coef_bytes * FRAMES + planes_bytes + rgb_bytes
    sets = CACHE_BYTES // per_set + 2
    # bits first
    views, _ = jpeg.fused_decode_batch(frames[:2], dev)
    want = jpeg.torch_jpeg_decode(header, coef)
    assert all(torch.equal(v.cpu(), want) for v in views), "device decode and restatement disagree"
    # the descriptor table and coefficients of each set, uploaded once
    n = FRAMES
    table_at = (header.coef_bytes * n + 15) // 16 * 16
    prepared = []
    for _ in range(sets):
        host = np.zeros(table_at + ctypes.sizeof(jpeg._Frame) * n, np.uint8)
        descs = (jpeg._Frame * n).from_buffer(host[table_at:])
        plane_at = 0
        for i, d in enumerate(descs):
            host[i * header.coef_bytes:(i + 1) * header.coef_bytes] = coef.view(np.uint8)
            d.width, d.height, d.hs, d.vs = header.width, header.height, header.hs[0], header.vs[0]
            for c in range(3):
                d.coef_off[c] = i * (header.coef_bytes // 2) + header.coef_offset[c]
                d.plane_off[c] = plane_at
                d.block_cols[c], d.block_rows[c] = header.block_cols[c], header.block_rows[c]
                plane_at += header.block_cols[c] * header.block_rows[c] * 64
            ctypes.memmove(d.quant, header.quant, ctypes.sizeof(header.quant))
            d.rgb_off = i * header.width * header.height * 3
        prepared.append((host, descs, torch.from_numpy(host).to(dev), torch.empty(planes_bytes, dtype=torch.uint8, device=dev),
                         torch.empty(rgb_bytes, dtype=torch.uint8, device=dev)))
    stream = _lib.stream_of(prepared[0][2])
    state = {"k": 0}

    def call():
        k = state["k"] = (state["k"] + 1) % sets
        _, descs, on_dev, planes, rgb = prepared[k]
        _lib.call("bfhip_jpeg_decode", ctypes.addressof(descs), on_dev.data_ptr() + table_at, n, on_dev.data_ptr(),
                  header.coef_bytes // 2 * n, planes.data_ptr(), planes.numel(), rgb.data_ptr(), rgb.numel(), stream)

    def window():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / CALLS

    for _ in range(WARMUP):
        window()
    ms = [window() for _ in range(TIMED)]
    nbytes = header.coef_bytes * n + 2 * planes_bytes + rgb_bytes
    rate = nbytes / (median(ms) * 1e-3)
    return dict(frames=n, both_launches_ms=round(median(ms), 5), both_launches_ms_min_max=[round(min(ms), 5), round(max(ms), 5)],
                ms_per_frame=round(median(ms) / n, 5),
                algorithmic_mb=dict(coefficients=round(header.coef_bytes * n / 1e6, 2), planes_written_and_read=round(2 * planes_bytes / 1e6, 2),
                                    rgb=round(rgb_bytes / 1e6, 2)),
                achieved_tb_per_s=round(rate / 1e12, 3), hbm_peak_share=round(rate / HBM_BYTES_PER_S, 3), buffer_sets=sets,
                calls_per_window=CALLS, warmup_windows=WARMUP, timed_windows=TIMED, bits_equal=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_micro.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--rows=")), "host,device").split(",")
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "jpeg_micro.json"))
    data = open(FIXTURE, "rb").read()
    header, coef = jpeg.entropy_decode(data)
    line = dict(frame=os.path.basename(FIXTURE), file_bytes=len(data), size=[header.width, header.height],
                sampling="%dx%d" % (header.hs[0], header.vs[0]), gpu=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM_BYTES_PER_S,
                upload=dict(coefficient_mb_per_frame=round(header.coef_bytes / 1e6, 3),
                            decoded_mb_per_frame=round(header.width * header.height * 3 / 1e6, 3),
                            ratio=round(header.coef_bytes / (header.width * header.height * 3), 3)),
                host=host_row(data) if "host" in rows else None,
                device=device_row(dev, header, coef) if "device" in rows else None)
    print(json.dumps(line), flush=True)
    with open(out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
