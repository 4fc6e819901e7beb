#!/usr/bin/env python3
"""The prediction visualiser on the device: bevfusion_amd.visualize (csrc/visualize.hip) against (a) its torch specification on
the same GPU and (b), where matplotlib is importable, a restatement of the reference tools' plotting calls on one host core.

Shapes: 6 x 900 x 1600 frames of the nominal rig already on the device, 200 and 500 boxes, scale 1 and 3; a 260 000-point
sweep already on the device on the reference's 1000 x 1000 BEV canvas with the same boxes.  Per shape one JSON entry:

  kernel        render_cameras / render_bev as a user calls them: box table on the host, one pinned upload, the launches, the
                output allocation; a host clock round the call and a device synchronise.  Median of TIMED calls after WARMUP.
  launches      device events round each bfhip_vis_* entry inside those calls (median): the segment set-up and the composite
                (cameras), the point scatter, the set-up and the composite (BEV).  composite_hbm_fraction = (one read of the
                frames + one write of the mosaic) / composite time / 8 TB/s, the HBM3E peak of MI355X_MICROARCH.md.
  torch         the same call with the specification (BFHIP_VISUALIZE=0) on the same device; median of SPEC_REPEATS.
  matplotlib    imshow + one ax.plot per edge on a 2 x 3 grid of axes, tight_layout, canvas.draw (cameras); scatter + one
                plt.plot per footprint at dpi = 10 (BEV): the reference's calls, Agg backend, one call each.

The kernel's image is compared with the specification's first (torch.equal).  A missing GPU is an error.
Usage: visualize_micro.py [OUT.json]   (default OUT: profiles/visualize_micro.json)"""
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
from bevfusion_amd import visualize as vz

WARMUP, TIMED, SPEC_REPEATS = 5, 300, 3
HBM_PEAK = 8.0e12
EVENTS = {}


def timed_call(name, *args):
    if not name.startswith("bfhip_vis_") or not torch.cuda.is_available():
        return _ORIG_CALL(name, *args)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    _ORIG_CALL(name, *args)
    b.record()
    EVENTS.setdefault(name, []).append((a, b))


_ORIG_CALL = _lib.call


def median_ms(fn, warmup, timed):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(timed):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(out)), 3), [round(min(out), 3), round(max(out), 3)]


def launch_times():
    torch.cuda.synchronize()
    out = {name: round(float(np.median([a.elapsed_time(b) for a, b in pairs])), 4) for name, pairs in EVENTS.items()}
    EVENTS.clear()
    return out


def matplotlib_cameras(frames, boxes, colors, l2c, K):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    corners = vz.box_corners(boxes)
    uv, z = vz.project_corners(corners, l2c, K)
    t = time.perf_counter()
    fig, axs = plt.subplots(2, 3, figsize=(15, 8))
    for v, ax in enumerate(np.array(axs).reshape(-1)):
        ax.imshow(frames[v])
        for i in range(len(boxes)):
            if not (z[v, i] > 0).any():
                continue
            for a, b in vz.EDGES:
                if uv[v, i, a, 0] < -10000 or uv[v, i, b, 0] < -10000:
                    continue
                ax.plot([uv[v, i, a, 0], uv[v, i, b, 0]], [uv[v, i, a, 1], uv[v, i, b, 1]], color=colors[i] / 255.0, linewidth=2)
        ax.axis("off")
    plt.tight_layout()
    fig.canvas.draw()
    np.array(fig.canvas.renderer.buffer_rgba())
    plt.close(fig)
    return round((time.perf_counter() - t) * 1e3, 1)


def matplotlib_bev(points, boxes, colors, path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    coords = vz.box_corners(boxes)[:, [0, 3, 7, 4, 0], :2]
    t = time.perf_counter()
    fig = plt.figure(figsize=(100, 100))
    ax = plt.gca()
    ax.set_xlim(-50, 50)
    ax.set_ylim(-50, 50)
    ax.set_aspect(1)
    ax.set_axis_off()
    plt.scatter(points[:, 0], points[:, 1], s=15, c="white")
    for i in range(len(coords)):
        plt.plot(coords[i, :, 0], coords[i, :, 1], linewidth=25, color=colors[i] / 255.0)
    fig.savefig(fname=path, dpi=10, facecolor="black", format="png", bbox_inches="tight", pad_inches=0)
    plt.close()
    return round((time.perf_counter() - t) * 1e3, 1)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "visualize_micro.json")
    if not torch.cuda.is_available():
        raise SystemExit("visualize_micro.py needs a GPU")
    try:
        import matplotlib  # noqa: F401
        have_mpl = True
    except ImportError:
        have_mpl = False
    dev = torch.device("cuda:0")
    _lib.call = timed_call
    rig = synthetic.camera_rig(batch=1)
    l2c, K = np.linalg.inv(rig["camera2lidar"][0].astype(np.float64)), rig["camera_intrinsics"][0]
    frames_h = synthetic.camera_images_u8(batch=1, views=6, h=900, w=1600, seed=2001)[0].transpose(0, 2, 3, 1).copy()
    frames = torch.from_numpy(frames_h).to(dev)
    points_h = synthetic.lidar_sweep(260000, seed=1000)
    points = torch.from_numpy(points_h).to(dev)
    results = []
    for n in (200, 500):
        boxes, _ = synthetic.gt_boxes(seed=3000 + n, n=n)
        colors = np.random.RandomState(n).randint(0, 256, (n, 3)).astype(np.uint8)
        mpl_cam = matplotlib_cameras(frames_h, boxes, colors, l2c, K) if have_mpl else None
        for scale in (1, 3):
            kw = dict(frames=frames, boxes=boxes, colors=colors, lidar2cam=l2c, cam2img=K, scale=scale)
            vz.ENABLED = True
            got = vz.render_cameras(**kw)
            EVENTS.clear()
            k_ms, k_mm = median_ms(lambda: vz.render_cameras(**kw), WARMUP, TIMED)
            launches = launch_times()
            vz.ENABLED = False
            want = vz.render_cameras(**kw)
            s_ms, s_mm = median_ms(lambda: vz.render_cameras(**kw), 0, SPEC_REPEATS)
            comp = launches["bfhip_vis_composite"]
            nbytes = frames.numel() + got.numel()
            results.append(dict(
                shape="cameras", frames=[6, 900, 1600], boxes=n, scale=scale, device=torch.cuda.get_device_name(0), warmup_calls=WARMUP,
                timed_calls=TIMED, kernel=dict(ms_per_call=k_ms, min_max=k_mm, launches=2),
                launches_ms=dict(segment_setup=launches["bfhip_vis_camera_segments"], composite=comp),
                composite_algorithmic_bytes=nbytes, composite_hbm_fraction=round(nbytes / (comp * 1e-3) / HBM_PEAK, 4),
                torch=dict(ms_per_call=s_ms, min_max=s_mm, calls=SPEC_REPEATS, device="the same GPU"),
                matplotlib=dict(ms_per_call=mpl_cam, threads=1, calls=1, note="full resolution; it has no scale") if have_mpl else "not importable",
                speedup_vs_torch=round(s_ms / k_ms, 1), kernel_faster=bool(k_ms < s_ms), bit_equal=bool(torch.equal(got, want))))
            print(json.dumps(results[-1]), flush=True)
        kw = dict(points=points, boxes=boxes, colors=colors)
        vz.ENABLED = True
        got = vz.render_bev(**kw)
        EVENTS.clear()
        k_ms, k_mm = median_ms(lambda: vz.render_bev(**kw), WARMUP, TIMED)
        launches = launch_times()
        vz.ENABLED = False
        want = vz.render_bev(**kw)
        s_ms, s_mm = median_ms(lambda: vz.render_bev(**kw), 0, SPEC_REPEATS)
        mpl = matplotlib_bev(points_h, boxes, colors, os.path.join(os.path.dirname(out_path), ".visualize_micro_bev.png")) if have_mpl else None
        if have_mpl:
            os.remove(os.path.join(os.path.dirname(out_path), ".visualize_micro_bev.png"))
        results.append(dict(
            shape="bev", canvas=[1000, 1000], points=260000, boxes=n, device=torch.cuda.get_device_name(0), warmup_calls=WARMUP,
            timed_calls=TIMED, kernel=dict(ms_per_call=k_ms, min_max=k_mm, launches="memset + 3"),
            launches_ms=dict(points=launches["bfhip_vis_bev_points"], segment_setup=launches["bfhip_vis_bev_segments"],
                             composite=launches["bfhip_vis_composite"]),
            torch=dict(ms_per_call=s_ms, min_max=s_mm, calls=SPEC_REPEATS, device="the same GPU"),
            matplotlib=dict(ms_per_call=mpl, threads=1, calls=1) if have_mpl else "not importable",
            speedup_vs_torch=round(s_ms / k_ms, 1), kernel_faster=bool(k_ms < s_ms), bit_equal=bool(torch.equal(got, want))))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")
    return 0 if all(r["bit_equal"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
