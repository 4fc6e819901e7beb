#!/usr/bin/env python3
"""JPEG encode of the visualiser's frames: the device path (csrc/jpeg_encode.hip) against the host path of the same module and
against Pillow on one core.

Frames: the 1800 x 4800 camera mosaic and the 1000 x 1000 BEV plot of one full-size synthetic sample of tools/visualize.py,
rendered on the GPU; quality 90, 4:2:0, a restart marker every MCU row.  One JSON object, per frame:

  device_launches    (a) HIP events around CALLS back-to-back calls of bfhip_jpeg_encode (three launches; descriptor table uploaded
                     before), median and min .. max of TIMED windows after WARMUP.  Every call takes the next of SETS pixel /
                     coefficient / workspace / output buffer sets whose total exceeds the 256 MiB Infinity Cache.
  device_end_to_end  (b) host clock round jpeg_encode.fused_jpeg_encode on the device tensor: buffers, the table's upload, the three
                     launches, the read of the length, the copy of exactly that many bytes, the markers; median, min .. max.
  host_path          (c) the copy of the RGB frame to the host plus jpeg_encode.encode (numpy + the C++ entropy stage), one thread.
  pillow             (d) Image.save(quality=, subsampling=2, restart_marker_rows=1) of the same pixels on one core; null without PIL.
  stream_bytes       (e) the file's size, and the pixels' for comparison.

The device bytes are asserted equal to the host path's before anything is timed.  A missing GPU is an error.
Usage: jpeg_encode_micro.py [--rows=device,host] [OUT.json]  (default OUT: profiles/jpeg_encode_micro.json)"""
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
from bevfusion_amd import jpeg_encode as je
from bevfusion_amd import visualize as vz

CACHE_BYTES = 256 << 20
CALLS, WARMUP, TIMED = 10, 5, 30
E2E_REPEATS, HOST_REPEATS = 15, 3
QUALITY, SUBSAMPLING = 90, "4:2:0"


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def spread(ms, key="ms"):
    return {key: round(median(ms), 4), key + "_min_max": [round(min(ms), 4), round(max(ms), 4)]}


def rendered_frames(dev):
    import visualize as tool
    meta, frames, points, what = next(iter(tool.synthetic_samples(1, small=False)))
    mosaic, bev = vz.visualize_sample(meta, torch.from_numpy(np.ascontiguousarray(frames)).to(dev),
                                      torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev), what, tool.NUSC_CLASSES)
    return [("camera_mosaic", mosaic.contiguous()), ("bev_plot", bev.contiguous())]


def launches_row(frame):
    h, w = frame.shape[:2]
    spec = [(w, h) + je.SAMPLINGS[SUBSAMPLING] + (je.quant_tables(QUALITY),)]
    probe = je.EncodeBatch(spec, frame.device)
    per_set = probe.rgb_bytes + probe.coef_elems * 2 + probe.ws_bytes + probe.out_bytes
    sets = CACHE_BYTES // per_set + 2
    prepared = []
    for _ in range(sets):
        batch = je.EncodeBatch(spec, frame.device)
        batch.upload()
        batch.alloc()
        prepared.append((batch, frame.clone().view(-1)))
    state = {"k": 0}

    def call():
        k = state["k"] = (state["k"] + 1) % sets
        prepared[k][0].encode(prepared[k][1])

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
    row = spread(ms, "three_launches_ms")
    row.update(pixels_mb_per_s=round(h * w * 3 / 1e6 / (median(ms) * 1e-3), 1), buffer_sets=sets, workspace_mb=round(probe.ws_bytes / 1e6, 2),
               calls_per_window=CALLS, warmup_windows=WARMUP, timed_windows=TIMED)
    return row


def timed_host(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def frame_rows(name, frame, rows):
    h, w = frame.shape[:2]
    device_bytes = je.fused_jpeg_encode([frame], QUALITY, SUBSAMPLING)[0]
    host_bytes = je.encode(frame.cpu().numpy(), QUALITY, SUBSAMPLING, 1)
    assert device_bytes == host_bytes, "%s: the device path's bytes are not the host path's" % name
    out = dict(size=[w, h], bytes_equal_host_path=True,
               stream_bytes=dict(file=len(device_bytes), pixels=h * w * 3, ratio=round(len(device_bytes) / (h * w * 3), 4)))
    if "device" in rows:
        out["device_launches"] = launches_row(frame)

        def e2e():
            je.fused_jpeg_encode([frame], QUALITY, SUBSAMPLING)  # ends in the copy of the stream: synchronous
        torch.cuda.synchronize()
        out["device_end_to_end"] = spread(timed_host(e2e, E2E_REPEATS))
    if "host" in rows:
        torch.set_num_threads(1)
        out["host_path"] = dict(threads=1, repeats=HOST_REPEATS, **spread(timed_host(
            lambda: je.encode(frame.cpu().numpy(), QUALITY, SUBSAMPLING, 1), HOST_REPEATS)))
        try:
            import io
            from PIL import Image
            pixels = frame.cpu().numpy()

            def pillow():
                Image.fromarray(pixels).save(io.BytesIO(), "JPEG", quality=QUALITY, subsampling=2, restart_marker_rows=1)
            out["pillow"] = dict(threads=1, repeats=HOST_REPEATS * 3, **spread(timed_host(pillow, HOST_REPEATS * 3)))
        except ImportError:
            out["pillow"] = None
    return out


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_encode_micro.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--rows=")), "device,host").split(",")
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "jpeg_encode_micro.json"))
    line = dict(gpu=torch.cuda.get_device_name(0), quality=QUALITY, subsampling=SUBSAMPLING, restart_rows=1)
    for name, frame in rendered_frames(dev):
        line[name] = frame_rows(name, frame, rows)
        print(json.dumps({name: line[name]}), flush=True)
    with open(out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
