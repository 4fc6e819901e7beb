#!/usr/bin/env python3
"""Writes tests/golden/jpeg_cases.npz and tests/golden/nus_cam_front.jpg for tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py and
tests/test_camera_load_cpu.py.  Needs PIL; sections (b) and (c) need REFERENCE_ROOT (default /root/reference).

(a) Synthetic streams (tests/jpeg_cases.py: synthetic_specs): tiny JPEGs Pillow writes from seeded noise mixed with gradients,
    each with Pillow's decoded pixels.  4:2:0 at 17x23, 33x9, 16x16 and 1x1, 4:2:2 at 19x10, 4:4:4 at 9x7, each at quality
    30 / 75 / 100; one optimize=True stream and one with restart_marker_blocks=2 (asserted to hold a DRI segment).
(b) The reference's smallest demo frame (CAM_FRONT) copied as data; the SHA-256 of Pillow's decode and three 32x32 windows.
(c) The reference's own BEVLoadMultiViewImageFromFiles.transform on the demo .pkl: its loading.py is loaded at run time by
    file path behind stubs (mmcv.imfrombytes = Pillow's decode, which is what its pillow backend is; mmcv.impad;
    mmengine.fileio.get = a file read; the mmdet3d base class keeps the keywords); nothing of it is copied.  Recorded: the
    inputs (cam2img, lidar2cam per camera), every matrix key and the shape keys; and for the num_ref_frames branch, per
    (seed, frames, num_ref_frames, test_mode), the chosen frames, the kept ego2global rows and the next np.random.uniform().
(d) Streams the fused decoder does not take: Pillow's progressive and grayscale output."""
import copy
import hashlib
import importlib.util
import json
import os
import pickle
import shutil
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases as jc  # noqa: E402

ROOT = os.environ.get("REFERENCE_ROOT", "/root/reference")
REF = os.path.join(ROOT, "projects", "BEVFusion", "bevfusion", "loading.py")
DEMO = os.path.join(ROOT, "demo", "data", "nuscenes")
REF_FRAME_CASES = [(seed, frames, refs, test_mode) for seed in (0, 1, 2) for (frames, refs) in ((1, 2), (3, 2), (4, 3), (2, 3))
                   for test_mode in (False, True)]


def load_reference():
    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    class _Base:
        def __init__(self, to_float32=False, color_type="unchanged", backend_args=None, num_views=5, num_ref_frames=-1,
                     test_mode=False, set_default_scale=True):
            self.to_float32, self.color_type, self.backend_args = to_float32, color_type, backend_args
            self.num_views, self.num_ref_frames = num_views, num_ref_frames
            self.test_mode, self.set_default_scale = test_mode, set_default_scale

    def imfrombytes(content, flag="color", channel_order="bgr", backend=None):
        assert backend == "pillow" and channel_order == "rgb"
        return jc.pillow_decode(content)

    def impad(img, shape=None, pad_val=0):
        out = np.full((shape[0], shape[1]) + img.shape[2:], pad_val, dtype=img.dtype)
        out[:img.shape[0], :img.shape[1]] = img
        return out

    def get(name, backend_args=None):
        with open(name, "rb") as f:
            return f.read()

    stubs = {"mmcv": dict(imfrombytes=imfrombytes, impad=impad), "mmengine": {}, "mmengine.fileio": dict(get=get),
             "mmdet3d": {}, "mmdet3d.datasets": {}, "mmdet3d.datasets.transforms": dict(LoadMultiViewImageFromFiles=_Base),
             "mmdet3d.registry": dict(TRANSFORMS=_Registry())}
    for name, attrs in stubs.items():
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.__dict__.update(attrs)
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_loading", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.BEVLoadMultiViewImageFromFiles


def has_marker(data, marker):
    return bytes([0xFF, marker]) in data


def main():
    out = {}
    # (a)
    names = []
    for name, seed, w, h, sub, q, kw in jc.synthetic_specs():
        data = jc.encode(jc.picture(seed, w, h), q, sub, **kw)
        if "restart_marker_blocks" in kw:
            assert has_marker(data, 0xDD), "no DRI segment"
        assert has_marker(data, 0xC0) and not has_marker(data, 0xC2)
        pixels = jc.pillow_decode(data)
        assert pixels.shape == (h, w, 3)
        out["stream_%s_bytes" % name] = np.frombuffer(data, np.uint8)
        out["stream_%s_pixels" % name] = pixels
        names.append(name)
    out["stream_names"] = np.array(json.dumps(names))
    # (d)
    pic = jc.picture(900, 24, 20)
    unsupported = {"progressive": jc.encode(pic, 75, 2, progressive=True)}
    buf = __import__("io").BytesIO()
    Image.fromarray(pic).convert("L").save(buf, "JPEG", quality=75)
    unsupported["grayscale"] = buf.getvalue()
    assert has_marker(unsupported["progressive"], 0xC2)
    for name, data in unsupported.items():
        out["unsupported_%s_bytes" % name] = np.frombuffer(data, np.uint8)
        out["unsupported_%s_pixels" % name] = jc.pillow_decode(data)
    out["unsupported_names"] = np.array(json.dumps(sorted(unsupported)))
    # (b)
    with open([os.path.join(DEMO, f) for f in os.listdir(DEMO) if f.endswith(".pkl")][0], "rb") as f:
        info = pickle.load(f)["data_list"][0]
    front = os.path.join(DEMO, info["images"]["CAM_FRONT"]["img_path"])
    assert os.path.getsize(front) == min(os.path.getsize(os.path.join(DEMO, c["img_path"])) for c in info["images"].values())
    shutil.copyfile(front, jc.FIXTURE)
    pixels = jc.pillow_decode(open(jc.FIXTURE, "rb").read())
    H, W = pixels.shape[:2]
    out["fixture_shape"] = np.array([H, W], np.int64)
    out["fixture_sha256"] = np.array(hashlib.sha256(np.ascontiguousarray(pixels).tobytes()).hexdigest())
    out["fixture_window_top_left"] = pixels[:32, :32].copy()
    out["fixture_window_bottom_right"] = pixels[H - 32:, W - 32:].copy()
    out["fixture_window_centre"] = pixels[H // 2 - 16:H // 2 + 16, W // 2 - 16:W // 2 + 16].copy()
    # (c)
    cls = load_reference()
    cams = list(info["images"])
    out["transform_cams"] = np.array(json.dumps(cams))
    out["transform_in_cam2img"] = np.stack([np.array(info["images"][c]["cam2img"], np.float64) for c in cams])
    out["transform_in_lidar2cam"] = np.stack([np.array(info["images"][c]["lidar2cam"], np.float64) for c in cams])
    sample = copy.deepcopy(info)
    for c in cams:
        sample["images"][c]["img_path"] = os.path.join(DEMO, sample["images"][c]["img_path"])
    res = cls(to_float32=True, color_type="color", backend_args=None).transform(copy.deepcopy(sample))
    for key in ("cam2img", "lidar2cam", "cam2lidar", "lidar2img", "ori_cam2img"):
        out["transform_out_%s" % key] = res[key]
    out["transform_out_shapes"] = np.array(json.dumps(dict(
        img_shape=list(res["img_shape"]), ori_shape=list(res["ori_shape"]), pad_shape=list(res["pad_shape"]),
        scale_factor=res["scale_factor"], num_views=res["num_views"], num_ref_frames=res["num_ref_frames"],
        n_img=len(res["img"]), img_dtype=str(res["img"][0].dtype), img0_shape=list(res["img"][0].shape))))
    assert res["img"][0].dtype == np.float32 and np.array_equal(res["img"][0], pixels.astype(np.float32))
    V = 2
    small = dict(images={c: sample["images"][c] for c in cams[:V]})
    rows = []
    for seed, frames, refs, test_mode in REF_FRAME_CASES:
        rs = np.random.RandomState(50 + frames)
        d = copy.deepcopy(small)
        d["img_filename"] = ["%d_%d" % (f, v) for f in range(frames) for v in range(V)]
        d["ego2global"] = [np.eye(4) + 0.01 * rs.standard_normal((4, 4)) for _ in range(frames)]
        d["lidar2cam"] = [rs.standard_normal((4, 4)) for _ in range(frames * V)]
        d["cam2img"] = [rs.standard_normal((3, 3)) for _ in range(frames * V)]
        ego_in = np.stack(d["ego2global"])
        np.random.seed(seed)
        r = cls(num_views=V, num_ref_frames=refs, test_mode=test_mode).transform(d)
        nxt = np.random.uniform()
        choices = [int(n.split("_")[0]) for n in r["img_filename"][::V]]
        assert len(choices) == refs + 1 and choices[0] == 0
        assert np.array_equal(np.stack(r["ego2global"]), ego_in[choices])
        rows.append(dict(seed=seed, frames=frames, refs=refs, test_mode=test_mode, choices=choices, next_uniform=repr(nxt)))
    out["ref_frame_cases"] = np.array(json.dumps(rows))
    np.savez_compressed(jc.NPZ, **out)
    print(jc.NPZ, os.path.getsize(jc.NPZ), "bytes;", len(names), "streams;", jc.FIXTURE, os.path.getsize(jc.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
