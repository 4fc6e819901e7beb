#!/usr/bin/env python3
"""Writes tests/golden/image_aug.npz: the reference's own ImageAug3D (PIL pixels, its sampled parameters, its img_aug_matrix)
on seeded inputs, for tests/test_image_aug_cpu.py and tests/test_image_aug_gpu.py.

The reference's transforms_3d.py is loaded at run time from REFERENCE_ROOT (default /root/reference) behind stubs of the three
names it imports from packages that are not installed (mmcv.transforms.BaseTransform, mmdet3d.datasets.GlobalRotScaleTrans,
mmdet3d.registry.TRANSFORMS); nothing of it is copied.  Needs PIL.

Source 60 x 100, final_dim (16, 40), 3 cameras; TRAIN_SEEDS training draws (resize_lim [0.38, 0.55], rot_lim [-5.4, 5.4],
rand_flip) and one test draw.  The seeds are chosen so that a training draw resizes below 0.40: newW < 40, the crop hangs over
the right edge and the zero fill is in the data (asserted).  After each draw the next np.random.uniform() is recorded, so a
restatement can be held to the same number of generator calls."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.environ.get("REFERENCE_ROOT", "/root/reference"), "projects", "BEVFusion", "bevfusion", "transforms_3d.py")
H, W, FINAL, CAMS = 60, 100, (16, 40), 3
TRAIN_SEEDS = (0, 4, 7, 9)
TRAIN = dict(final_dim=FINAL, resize_lim=[0.38, 0.55], bot_pct_lim=[0.0, 0.0], rot_lim=[-5.4, 5.4], rand_flip=True, is_train=True)
TEST = dict(final_dim=FINAL, resize_lim=[0.38, 0.55], bot_pct_lim=[0.0, 0.0], rot_lim=[0.0, 0.0], rand_flip=False, is_train=False)


def load_reference():
    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    stubs = {"mmcv": {}, "mmcv.transforms": {"BaseTransform": object}, "mmdet3d": {},
             "mmdet3d.datasets": {"GlobalRotScaleTrans": object}, "mmdet3d.registry": {"TRANSFORMS": _Registry()}}
    for name, attrs in stubs.items():
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.__dict__.update(attrs)
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_transforms_3d", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ImageAug3D


def inputs():
    rs = np.random.RandomState(2024)
    frames = rs.randint(0, 256, (CAMS, H, W, 3)).astype(np.uint8)
    frames[:, 0, 0], frames[:, -1, -1] = 0, 255
    cam2img = np.tile(np.eye(4, dtype=np.float32), (CAMS, 1, 1))
    cam2lidar = np.tile(np.eye(4, dtype=np.float32), (CAMS, 1, 1))
    for i in range(CAMS):
        cam2img[i, 0, 0], cam2img[i, 1, 1] = 62.0 + i, 61.0 - i
        cam2img[i, 0, 2], cam2img[i, 1, 2] = 49.5 + 0.5 * i, 30.0 - i
        # third row of the camera -> lidar rotation: a camera looking level (i = 0: horizon above the image centre),
        # pitched down and rolled (i = 1) and pitched up (i = 2: horizon below, yh > 0 and the top is cropped away)
        cam2lidar[i, 2, :3] = [(0.0, -1.0, 0.02), (0.03, -0.99, 0.12), (-0.02, -0.99, -0.2)][i]
    return frames, cam2img, cam2lidar


def main():
    cls = load_reference()
    frames, cam2img, cam2lidar = inputs()
    out = dict(frames=frames, cam2img=cam2img, cam2lidar=cam2lidar, ori_shape=np.array([H, W]), final_dim=np.array(FINAL))
    draws = [(s, TRAIN) for s in TRAIN_SEEDS] + [(0, TEST)]
    narrow = False
    for d, (seed, cfg) in enumerate(draws):
        aug = cls(**cfg)
        data = dict(ori_shape=(H, W), cam2img=cam2img, cam2lidar=cam2lidar)
        np.random.seed(seed)
        params = [aug.sample_augmentation(data, i) for i in range(CAMS)]
        data["img"] = [f.astype(np.float32) for f in frames]  # the loader hands float32 arrays over
        np.random.seed(seed)
        res = aug.transform(data)
        nxt = np.random.uniform()
        pix = np.stack(res["img"])
        assert pix.dtype == np.float32 and np.array_equal(pix, pix.astype(np.uint8))
        out["draw%d_seed" % d] = np.array(seed)
        out["draw%d_train" % d] = np.array(cfg["is_train"])
        out["draw%d_resize" % d] = np.array([p[0] for p in params], np.float64)
        out["draw%d_dims" % d] = np.array([p[1] for p in params], np.int64)
        out["draw%d_crop" % d] = np.array([p[2] for p in params], np.int64)
        out["draw%d_flip" % d] = np.array([p[3] for p in params], np.bool_)
        out["draw%d_rotate" % d] = np.array([p[4] for p in params], np.float64)
        out["draw%d_matrix" % d] = np.stack(res["img_aug_matrix"]).astype(np.float32)
        out["draw%d_img" % d] = pix.astype(np.uint8)
        out["draw%d_next_uniform" % d] = np.array(nxt, np.float64)
        narrow = narrow or any(p[1][0] < FINAL[1] for p in params)
    assert narrow, "no draw with newW < fW: choose other seeds"
    out["n_draws"] = np.array(len(draws))
    path = os.path.join(HERE, "image_aug.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
