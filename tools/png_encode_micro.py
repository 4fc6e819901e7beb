#!/usr/bin/env python3
"""PNG encode of the visualiser's frames: the device path (csrc/png_encode.hip) against the host path of the same module and
against Pillow on one core.

Frames: the 1800 x 4800 camera mosaic and the 1000 x 1000 BEV plot of one full-size synthetic sample of tools/visualize.py,
rendered on the GPU; default band size.  One JSON object, per frame:

  device_launches    (a) HIP events around CALLS back-to-back calls of bfhip_png_encode (four launches; descriptor table uploaded
                     before), median and min .. max of TIMED windows after WARMUP.  Every call takes the next of SETS pixel /
                     workspace / output buffer sets whose total exceeds the 256 MiB Infinity Cache.
  kernels            (b) per kernel, from one torch.profiler trace of CALLS such calls: device time, the algorithmic bytes (pixels in,
                     filtered bytes written and read, stream out) and the fraction of the HBM peak they amount to; null when the
                     profiler reports no kernels.
  device_end_to_end  (c) host clock round png_encode.fused_png_encode on the device tensor: buffers, the table's upload, the four
                     launches, the one read (lengths, flags, Adler triples), the copy of exactly that many bytes, the chunks and
                     their CRCs; median, min .. max.
  host_path          (d) the copy of the RGB frame to the host plus png_encode.encode (the C++ filter and deflate), one thread.
  pillow             (e) the same copy plus Image.save at Pillow's default level and at compress_level=1, one core; null without PIL.
  file_bytes         (f) the size of each file, and the pixels' for comparison.

The device bytes are asserted equal to the host path's, and the decoded pixels to the frame, before anything is timed.  A
missing GPU is an error.
Usage: png_encode_micro.py [--rows=device,kernels,host] [OUT.json]  (default OUT: profiles/png_encode_micro.json)"""
import io
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
from bevfusion_amd import png_encode as pe
from bevfusion_amd import visualize as vz

CACHE_BYTES = 256 << 20
HBM_PEAK = 8.0e12  # bytes/s, MI355X
CALLS, WARMUP, TIMED = 10, 5, 30
E2E_REPEATS, HOST_REPEATS = 15, 3


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


def prepared_sets(frame):
    h, w = frame.shape[:2]
    probe = pe.EncodeBatch([(w, h, None)], frame.device)
    per_set = probe.src_bytes + probe.ws_bytes + probe.out_bytes
    sets = CACHE_BYTES // per_set + 2
    return probe, [(pe.EncodeBatch([(w, h, None)], frame.device), frame.clone().view(-1)) for _ in range(sets)]


def launches_row(frame, prepared, probe):
    h, w = frame.shape[:2]
    sets = len(prepared)
    state = {"k": 0}

    def call():
        k = state["k"] = (state["k"] + 1) % sets
        prepared[k][0].run(prepared[k][1])

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
    row = spread(ms, "four_launches_ms")
    row.update(pixels_mb_per_s=round(h * w * 3 / 1e6 / (median(ms) * 1e-3), 1), buffer_sets=sets, workspace_mb=round(probe.ws_bytes / 1e6, 2),
               bands=int(-(-probe.descs[0].n_bytes // probe.descs[0].band_bytes)), band_bytes=int(probe.descs[0].band_bytes),
               calls_per_window=CALLS, warmup_windows=WARMUP, timed_windows=TIMED)
    return row, call


def kernels_row(call, pixels, filtered, stream):
    """Device time per kernel from one profiler trace; the algorithmic bytes are what the stage must move at the least."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(CALLS):
            call()
        torch.cuda.synchronize()
    traffic = {"png_filter_kernel": pixels + filtered, "png_band_kernel": 2 * filtered + stream, "png_offsets_kernel": 0,
               "png_compact_kernel": 2 * stream}
    rows = {}
    for ev in prof.key_averages():
        for name, moved in traffic.items():
            if name in ev.key:
                us = float(getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)) / max(ev.count, 1)
                if us > 0:
                    rows[name] = dict(us=round(us, 2), calls=int(ev.count), algorithmic_bytes=int(moved),
                                      hbm_peak_fraction=round(moved / (us * 1e-6) / HBM_PEAK, 4))
    return rows or None


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
    device_bytes = pe.fused_png_encode([frame])[0]
    host_bytes = pe.encode(frame.cpu().numpy())
    assert device_bytes == host_bytes, "%s: the device path's bytes are not the host path's" % name
    sizes = dict(this_module=len(device_bytes), pixels=h * w * 3)
    out = dict(size=[w, h], bytes_equal_host_path=True, file_bytes=sizes)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(device_bytes)).convert("RGB")), frame.cpu().numpy()), name
        out["decodes_to_the_frame"] = True
    if "device" in rows or "kernels" in rows:
        probe, prepared = prepared_sets(frame)
        out["device_launches"], call = launches_row(frame, prepared, probe)
        if "kernels" in rows:
            try:
                out["kernels"] = kernels_row(call, h * w * 3, int(probe.descs[0].n_bytes), len(device_bytes))
            except Exception as e:  # the profiler is an observer: the other rows stand without it
                out["kernels"] = dict(error=repr(e))

        def e2e():
            pe.fused_png_encode([frame])  # ends in the copy of the stream: synchronous
        torch.cuda.synchronize()
        out["device_end_to_end"] = spread(timed_host(e2e, E2E_REPEATS))
    if "host" in rows:
        torch.set_num_threads(1)
        out["host_path"] = dict(threads=1, repeats=HOST_REPEATS, **spread(timed_host(lambda: pe.encode(frame.cpu().numpy()), HOST_REPEATS)))
        if Image is None:
            out["pillow"] = None
        else:
            out["pillow"] = {}
            for key, kw in (("default", {}), ("compress_level_1", dict(compress_level=1))):
                buf = io.BytesIO()
                Image.fromarray(frame.cpu().numpy()).save(buf, "PNG", **kw)
                sizes["pillow_" + key] = len(buf.getvalue())
                out["pillow"][key] = dict(threads=1, repeats=HOST_REPEATS, **spread(timed_host(
                    lambda kw=kw: Image.fromarray(frame.cpu().numpy()).save(io.BytesIO(), "PNG", **kw), HOST_REPEATS)))
            sizes["ratio_to_pillow_default"] = round(len(device_bytes) / sizes["pillow_default"], 4)
    return out


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("png_encode_micro.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--rows=")), "device,kernels,host").split(",")
    out = next((a for a in sys.argv[1:] if a.endswith(".json")), os.path.join(ROOT, "profiles", "png_encode_micro.json"))
    line = dict(gpu=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK)
    for name, frame in rendered_frames(dev):
        line[name] = frame_rows(name, frame, rows)
        print(json.dumps({name: line[name]}), flush=True)
    with open(out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")
