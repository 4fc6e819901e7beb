#!/usr/bin/env python3
"""Draws saved predictions: per sample a camera mosaic and a bird's-eye plot, written as PNG frames and, with --video, as a Motion-JPEG AVI.

    visualize.py RESULTS.pkl ANN_FILE --out DIR [--data-root ROOT] [--classes car,truck,...] [--threshold 0.01] [--gt]
                 [--only-classes car truck] [--cam-order 0 1 2] [--scale 3] [--max-vis 10] [--no-track] [--device cuda:0|cpu]
                 [--video OUT.avi] [--fps 2] [--quality 90] [--video-stream cameras|bev] [--no-png] [--png-encoder pillow|device]
    visualize.py --synthetic --out DIR [--frames 3] [--scale 3] [--small]

RESULTS.pkl: the list tools/evaluate.py takes, one entry per sample with 'sample_idx' and 'pred_instances_3d' {'bboxes_3d',
'scores_3d', 'labels_3d'} (or the three keys directly).  ANN_FILE: the infos (.pkl or .json with a `data_list`); entry
`sample_idx` names the camera files (`images`: img_path, lidar2cam, cam2img) and the sweep (`lidar_points`: lidar_path,
num_pts_feats), relative to --data-root.  --gt draws the infos' `instances` instead of the predictions (no tracking), as the
reference tool does without --show-pred.  Predictions pass a score threshold, the class filter and the light tracker
(bevfusion_amd.visualize.Tracker3D).  Out: DIR/cameras/000000.png ... and DIR/bev/000000.png ..., written with Pillow
(--no-png: not written); --png-encoder device writes them with bevfusion_amd.png_encode instead: lossless too, the same pixels in a
file of its own making, encoded on the device from the tensor the renderer left there, without copying the pixels to the host
(on a machine without a GPU its host path writes the same bytes).  --video OUT.avi also writes the camera mosaics (--video-stream bev: the BEV plots) as a video, as the
reference tools do -- they encode mp4v into an mp4 with OpenCV; here every frame is a baseline JPEG, encoded on the device from
the tensor the renderer left there (bevfusion_amd.jpeg_encode.encode_frames), in an AVI file (MjpegAviWriter).
--synthetic draws seeded frames, sweeps and boxes of the nominal six-camera rig instead (--small: 90 x 160 frames)."""
import argparse
import json
import os
import pickle
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import jpeg_encode
from bevfusion_amd import png_encode
from bevfusion_amd import synthetic
from bevfusion_amd import visualize as vz

NUSC_CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]


def synthetic_samples(n_frames, small=False, seed=0):
    """Seeded samples of the nominal rig: (meta, frames uint8 [6, H, W, 3], points [m, 5], pred) per frame; the boxes drift so
    that the tracker has something to follow."""
    rig = synthetic.camera_rig(batch=1)
    H, W, div = (90, 160, 10.0) if small else (900, 1600, 1.0)
    K = rig["camera_intrinsics"][0].copy()
    K[:, :2, :3] /= div
    meta = dict(ori_cam2img=K, lidar2cam=np.linalg.inv(rig["camera2lidar"][0].astype(np.float64)))
    boxes, labels = synthetic.gt_boxes(seed=3000 + seed, n=24)
    rs = np.random.RandomState(seed)
    scores = rs.uniform(0.05, 0.95, len(boxes)).astype(np.float32)
    for i in range(n_frames):
        frames = synthetic.camera_images_u8(batch=1, views=6, h=H, w=W, seed=2000 + i)[0].transpose(0, 2, 3, 1).copy()
        points = synthetic.lidar_sweep(2000 if small else 40000, seed=1000 + i)
        moved = boxes[:, :7].copy()
        moved[:, 1] += 0.5 * i
        yield meta, frames, points, dict(bboxes_3d=moved, scores_3d=scores, labels_3d=labels)


def load_infos(path):
    with open(path, "rb") as f:
        infos = json.load(f) if path.endswith(".json") else pickle.load(f)
    return infos["data_list"] if isinstance(infos, dict) else infos


def real_samples(args):
    from bevfusion_amd import loading
    with open(args.results, "rb") as f:
        results = pickle.load(f)
    infos = load_infos(args.ann_file)
    by_idx = {info.get("sample_idx", i): info for i, info in enumerate(infos)}
    root = args.data_root or ""
    for r in results:
        info = by_idx[r["sample_idx"]]
        images = {k: dict(v, img_path=os.path.join(root, v["img_path"])) for k, v in info["images"].items() if v.get("img_path")}
        loaded = loading.BEVLoadMultiViewImageFromFiles(num_views=len(images)).transform(dict(images=images))
        frames = np.stack([np.asarray(im, np.uint8)[..., :3] for im in loaded["img"]], 0)
        meta = dict(ori_cam2img=loaded["ori_cam2img"], lidar2cam=loaded["lidar2cam"])
        points = None
        lp = info.get("lidar_points", {})
        if lp.get("lidar_path") and os.path.exists(os.path.join(root, lp["lidar_path"])):
            points = loading.read_points(os.path.join(root, lp["lidar_path"]), int(lp.get("num_pts_feats", 5)))
        if args.gt:
            inst = [i for i in info.get("instances", []) if i.get("bbox_label_3d", -1) >= 0]
            what = dict(gt_bboxes_3d=np.array([i["bbox_3d"] for i in inst], np.float32).reshape(-1, 7 if not inst else len(inst[0]["bbox_3d"])),
                        gt_labels_3d=np.array([i["bbox_label_3d"] for i in inst], np.int64))
        else:
            what = r.get("pred_instances_3d", r)
        yield meta, frames, points, what


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("results", nargs="?")
    ap.add_argument("ann_file", nargs="?")
    ap.add_argument("--out", required=True, help="output directory of the PNG frames")
    ap.add_argument("--video", default=None, metavar="PATH.avi",
                    help="also write the frames as a Motion-JPEG AVI (the reference tools write mp4v into an mp4)")
    ap.add_argument("--fps", type=float, default=2.0, help="frame rate of the video (the reference's: 2)")
    ap.add_argument("--quality", type=int, default=90, help="JPEG quality of the video's frames")
    ap.add_argument("--video-stream", choices=("cameras", "bev"), default="cameras")
    ap.add_argument("--no-png", action="store_true", help="with --video: write no PNG frames")
    ap.add_argument("--png-encoder", choices=("pillow", "device"), default="pillow",
                    help="who writes the PNG frames: Pillow from a host copy, or bevfusion_amd.png_encode from the device tensor")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--data-root", default=None)
    ap.add_argument("--classes", default=None)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--gt", action="store_true")
    ap.add_argument("--only-classes", nargs="*", default=None)
    ap.add_argument("--cam-order", type=int, nargs="*", default=None)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--max-vis", type=int, default=10, help="only the first K samples (-1: all)")
    ap.add_argument("--no-track", action="store_true")
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args(argv)
    if not args.synthetic and not (args.results and args.ann_file):
        ap.error("RESULTS.pkl and ANN_FILE, or --synthetic")
    if args.no_png and not args.video:
        ap.error("--no-png needs --video")
    if not args.no_png and args.png_encoder == "pillow":
        from PIL import Image
    classes = args.classes.split(",") if args.classes else NUSC_CLASSES
    dev = torch.device(args.device)
    tracker = None if (args.no_track or args.gt) else vz.Tracker3D(max_missed=3, max_dist=4.0)
    samples = synthetic_samples(args.frames, args.small) if args.synthetic else real_samples(args)
    written, writer = 0, None
    for i, (meta, frames, points, what) in enumerate(samples):
        if 0 <= args.max_vis <= i:
            break
        frames_t = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        points_t = None if points is None else torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
        mosaic, bev = vz.visualize_sample(meta, frames_t, points_t, what, classes, score_thr=args.threshold,
                                          only_classes=args.only_classes, tracker=tracker, cam_order=args.cam_order, scale=args.scale)
        shown = mosaic if args.video_stream == "cameras" else bev
        if args.video and shown is not None:
            data = jpeg_encode.encode_frames([shown], quality=args.quality)[0]  # from the device tensor on a GPU
            if writer is None:
                writer = jpeg_encode.MjpegAviWriter(args.video, args.fps, shown.shape[1], shown.shape[0])
            writer.write(data)
        todo = [(sub, img) for sub, img in (("cameras", mosaic), ("bev", bev)) if img is not None and not args.no_png]
        for sub, img in todo:
            os.makedirs(os.path.join(args.out, sub), exist_ok=True)
            if args.png_encoder == "pillow":
                Image.fromarray(img.cpu().numpy()).save(os.path.join(args.out, sub, "%06d.png" % i))
        if todo and args.png_encoder == "device":  # both images in one batch
            png_encode.write_frames([os.path.join(args.out, sub, "%06d.png" % i) for sub, _ in todo], [img for _, img in todo])
        written += 1
    if writer is not None:
        writer.close()
        print("%d frames in %s (%s path)" % (len(writer.index), args.video, "kernel" if jpeg_encode.PATHS["kernel"] else "host"))
    if args.png_encoder == "device" and not args.no_png:
        print("png: %s path" % ("kernel" if png_encode.PATHS["kernel"] else "host"))
    print("%d samples written under %s (%s path)" % (written, args.out, "kernel" if vz.PATHS["kernel"] else "host"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
