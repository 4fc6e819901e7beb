"""Shared by tests/test_multi_sweep_cpu.py and tests/test_multi_sweep_gpu.py: the recorded reference runs of
LoadPointsFromMultiSweeps (tests/golden/multi_sweep.npz, written by tests/golden/make_multi_sweep_golden.py), the fixture's
clouds written out as the .bin files the loaders read, and this package's transforms on the same inputs."""
import os

import numpy as np

from bevfusion_amd import points_aug as pa  # noqa: F401  registers the transforms
from bevfusion_amd.registry import TRANSFORMS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multi_sweep.npz")

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def names():
    return [str(n) for n in golden()["case_names"]]


def write_files(root):
    """The keyframe and the twelve sweeps as .bin files under `root` -> (keyframe path, the `lidar_sweeps` infos)."""
    g = golden()
    key_path = os.path.join(str(root), "keyframe.bin")
    g["keyframe"].tofile(key_path)
    starts = np.concatenate([[0], np.cumsum(g["sweep_counts"])])
    infos = []
    for i in range(len(g["sweep_counts"])):
        path = os.path.join(str(root), "sweep%d.bin" % i)
        g["sweep_points"][starts[i]:starts[i + 1]].tofile(path)
        infos.append(dict(lidar_points=dict(lidar_path=path, lidar2sensor=g["lidar2sensor"][i].tolist()),
                          timestamp=float(g["sweep_timestamps"][i])))
    return key_path, infos


def keywords(name):
    g = golden()
    pad, remove, test_mode = (bool(v) for v in g[name + "_flags"])
    return dict(sweeps_num=int(g["sweeps_num"]), load_dim=int(g["load_dim"]), use_dim=[int(d) for d in g[name + "_use_dim"]],
                pad_empty_sweeps=pad, remove_close=remove, test_mode=test_mode)


def frame(files, name):
    """The result dict the dataset hands to the pipeline for case `name`."""
    key_path, infos = files
    g = golden()
    data = dict(lidar_points=dict(lidar_path=key_path), timestamp=float(g["timestamp"]))
    if int(g[name + "_available"]) >= 0:
        data["lidar_sweeps"] = infos[:int(g[name + "_available"])]
    return data


def run(files, name, defer=False, after=(), tensor=False):
    """Case `name`: np.random.seed, LoadPointsFromFile -> LoadPointsFromMultiSweeps (+ the transforms `after`, dicts), built by
    name -> (data, the next np.random.uniform())."""
    import torch
    g = golden()
    np.random.seed(int(g[name + "_seed"]))
    load_dim = int(g["load_dim"])
    steps = [TRANSFORMS.build(dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=load_dim, use_dim=load_dim)),
             TRANSFORMS.build(dict(type="LoadPointsFromMultiSweeps", defer=defer, **keywords(name)))]
    steps += [TRANSFORMS.build(s) for s in after]
    data = frame(files, name)
    for i, t in enumerate(steps):
        data = t.transform(data)
        if i == 0 and tensor:
            data["points"] = torch.from_numpy(data["points"])
    return data, np.random.uniform()


def reference(name):
    """The reference's output of case `name`: [keyframe, column 4 zeroed ; the chosen sweeps' recorded rows][:, use_dim]."""
    g = golden()
    key0 = g["keyframe"].copy()
    key0[:, 4] = 0
    remove = bool(g[name + "_flags"][1])
    if int(g[name + "_available"]) < 0:
        rows = [key0] + [g["key_removed"]] * (int(g["sweeps_num"]) if bool(g[name + "_flags"][0]) else 0)
    else:
        rows = [key0] + [g[("piece%d" if remove else "raw_piece%d") % i] for i in g[name + "_choices"]]
    return np.concatenate(rows, 0)[:, [int(d) for d in g[name + "_use_dim"]]]
