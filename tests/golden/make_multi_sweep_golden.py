#!/usr/bin/env python3
"""Writes tests/golden/multi_sweep.npz: the reference's own LoadPointsFromMultiSweeps on a small seeded keyframe and twelve
sweeps, for tests/test_multi_sweep_cpu.py and tests/test_multi_sweep_gpu.py.

The reference's class is loaded at run time from REFERENCE_ROOT (default /root/reference) behind stubs of the packages that are
not installed (as make_object_sample_golden.py does); nothing of it is copied.  Real files: mmdet3d/utils/array_converter.py,
structures/bbox_3d/utils.py, structures/points/{base,lidar}_points.py, datasets/transforms/loading.py.  mmengine.fileio.get
is stubbed with a plain file read.

Inputs: a keyframe of N_KEY rows and N_SWEEPS sweeps of 150-400 rows, 5 floats per row; per sweep a rigid float64 lidar2sensor
(any rotation about z, a few degrees of roll and pitch, a translation of up to 8 m) and a timestamp.  Every cloud holds rows
inside the 1 m square, rows with |x| or |y| exactly 1.0 (which stay) and one NaN row (which stays).

Cases (CASES): train mode with 12 sweeps and sweeps_num=9 under several seeds, test_mode, 4 sweeps (fewer than sweeps_num), no
`lidar_sweeps` with pad_empty_sweeps True and False, remove_close=False, use_dim=[0, 1, 2, 4].  Per case np.random.seed(seed),
the transform is built and called once, then the next np.random.uniform() is recorded, and the sweeps it chose, in its order.

A case's output is [keyframe with column 4 zeroed ; the chosen sweeps' processed rows], and a sweep's processed rows do not
depend on the case; so the file records each sweep's processed rows ONCE (`piece%d`, with remove_close; `raw_piece%d` without,
for the sweeps that case reads; `key_removed`, the keyframe through remove_close) and per case the choices, and this script
asserts that every case's output is exactly that concatenation -- which keeps the file below 200 KB.

Asserted as well: the ordered float64 restatement -- float32((double(x) m0j + double(y) m1j) + double(z) m2j), then
float32(double(v) - t_j) -- reproduces every recorded value bit for bit; every sweep loses some but not all rows to
remove_close; the train cases choose different sweeps in different orders."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
N_KEY, N_SWEEPS, LOAD_DIM, SWEEPS_NUM = 600, 12, 5, 9
TIMESTAMP = 1533151603.547590
FULL = list(range(LOAD_DIM))
# name -> (seed, sweeps available (None: no `lidar_sweeps` key), keywords)
CASES = dict(
    train0=(0, 12, dict(use_dim=FULL, pad_empty_sweeps=True, remove_close=True)),
    train1=(1, 12, dict(use_dim=FULL, pad_empty_sweeps=True, remove_close=True)),
    train2=(2, 12, dict(use_dim=FULL, pad_empty_sweeps=True, remove_close=True)),
    test=(3, 12, dict(use_dim=FULL, pad_empty_sweeps=True, remove_close=True, test_mode=True)),
    few=(4, 4, dict(use_dim=FULL, pad_empty_sweeps=True, remove_close=True)),
    none_pad=(5, None, dict(use_dim=FULL, pad_empty_sweeps=True, remove_close=True)),
    none_nopad=(6, None, dict(use_dim=FULL, pad_empty_sweeps=False, remove_close=True)),
    noremove=(7, 4, dict(use_dim=FULL, pad_empty_sweeps=True, remove_close=False)),
    usedim=(8, 12, dict(use_dim=[0, 1, 2, 4], pad_empty_sweeps=True, remove_close=True)),
)


class _Any(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (object,), {})


class _Registry:
    def register_module(self, *a, **k):
        return lambda cls: cls


def _stub(name, **attrs):
    mod = _Any(name)
    mod.__dict__.update(attrs)
    mod.__path__ = []
    sys.modules[name] = mod
    return mod


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _get(path, backend_args=None):
    with open(path, "rb") as f:
        return f.read()


def load_reference():
    for name in ("cv2", "mmcv", "mmcv.transforms", "mmcv.transforms.base", "mmcv.ops", "mmdet", "mmdet.datasets",
                 "mmdet.datasets.transforms", "mmdet3d", "mmdet3d.structures", "mmdet3d.structures.bbox_3d", "mmengine"):
        _stub(name)
    _stub("mmengine.fileio", get=_get)
    _stub("mmdet3d.registry", TRANSFORMS=_Registry())
    ac = _load("mmdet3d.utils.array_converter", "mmdet3d/utils/array_converter.py")
    _stub("mmdet3d.utils", array_converter=ac.array_converter)
    ut = _load("mmdet3d.structures.bbox_3d.utils", "mmdet3d/structures/bbox_3d/utils.py")
    sys.modules["mmdet3d.structures.bbox_3d"].rotation_3d_in_axis = ut.rotation_3d_in_axis
    bp = _load("mmdet3d.structures.points.base_points", "mmdet3d/structures/points/base_points.py")
    lp = _load("mmdet3d.structures.points.lidar_points", "mmdet3d/structures/points/lidar_points.py")
    _stub("mmdet3d.structures.points", BasePoints=bp.BasePoints, LiDARPoints=lp.LiDARPoints,
          get_points_type=lambda coord_type: lp.LiDARPoints)
    ld = _load("mmdet3d.datasets.transforms.loading", "mmdet3d/datasets/transforms/loading.py")
    return lp.LiDARPoints, ld.LoadPointsFromMultiSweeps


def make_cloud(rs, n):
    """float32 [n, 5]: a ring of returns 2-50 m out, then rows inside the 1 m square, rows ON its border and a NaN row."""
    r, az = rs.uniform(2.0, 50.0, n), rs.uniform(-np.pi, np.pi, n)
    p = np.stack([r * np.cos(az), r * np.sin(az), rs.uniform(-3.0, 1.0, n), rs.uniform(0, 255, n), rs.uniform(0, 1, n)], 1)
    inside = max(8, n // 12)
    p[:inside, :2] = rs.uniform(-0.999, 0.999, (inside, 2))
    border = np.array([[1.0, 0.3], [-1.0, -0.5], [0.2, 1.0], [-0.7, -1.0], [1.0, 1.0], [-1.0, 1.0], [1.0, 40.0], [0.5, -30.0]])
    p[inside:inside + len(border), :2] = border  # the last two: one coordinate inside, the other far: they stay too
    p = p[rs.permutation(n)].astype(np.float32)
    p[n // 2, 0] = np.nan
    return p


def make_lidar2sensor(rs):
    yaw, pitch, roll = rs.uniform(-np.pi, np.pi), rs.uniform(-0.05, 0.05), rs.uniform(-0.05, 0.05)
    cz, sz, cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rot = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
           np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot, rs.uniform(-8.0, 8.0, 3)
    return m


def make_inputs():
    rs = np.random.RandomState(23)
    key = make_cloud(rs, N_KEY)
    sweeps = [make_cloud(rs, int(rs.randint(150, 401))) for _ in range(N_SWEEPS)]
    l2s = np.stack([make_lidar2sensor(rs) for _ in range(N_SWEEPS)])
    stamps = TIMESTAMP - 0.05 * (1 + np.arange(N_SWEEPS)) + rs.uniform(-0.004, 0.004, N_SWEEPS)
    return key, sweeps, l2s, stamps


def restate(p, m, dt, remove):
    """The ordered float64 restatement of one sweep."""
    if remove:
        p = p[~((np.abs(p[:, 0]) < 1.0) & (np.abs(p[:, 1]) < 1.0))]
    p = p.copy()
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    for j in range(3):
        v = ((x * m[0, j] + y * m[1, j]) + z * m[2, j]).astype(np.float32)
        p[:, j] = (v.astype(np.float64) - m[j, 3]).astype(np.float32)
    p[:, 4] = np.float32(dt)
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def main():
    LiDARPoints, Loader = load_reference()
    key, sweeps, l2s, stamps = make_inputs()
    out = dict(keyframe=key, sweep_points=np.concatenate(sweeps, 0), sweep_counts=np.array([len(s) for s in sweeps]),
               lidar2sensor=l2s, sweep_timestamps=stamps, timestamp=np.array(TIMESTAMP, np.float64), load_dim=np.array(LOAD_DIM),
               sweeps_num=np.array(SWEEPS_NUM), case_names=np.array(list(CASES)))
    key0 = key.copy()
    key0[:, 4] = 0
    pieces, raw_pieces, orders = {}, {}, []
    real_choice = np.random.choice
    with tempfile.TemporaryDirectory() as root:
        infos = []
        for i, s in enumerate(sweeps):
            path = os.path.join(root, "sweep%d.bin" % i)
            s.tofile(path)
            infos.append(dict(lidar_points=dict(lidar_path=path, lidar2sensor=l2s[i].tolist()), timestamp=float(stamps[i])))
        for name, (seed, available, kw) in CASES.items():
            chosen = []

            def choice(*a, **k):
                chosen.append(real_choice(*a, **k))
                return chosen[-1]

            np.random.seed(seed)
            np.random.choice = choice
            try:
                t = Loader(sweeps_num=SWEEPS_NUM, load_dim=LOAD_DIM, **kw)
                data = dict(points=LiDARPoints(torch.from_numpy(key.copy()), points_dim=LOAD_DIM), timestamp=TIMESTAMP)
                if available is not None:
                    data["lidar_sweeps"] = infos[:available]
                got = t.transform(data)["points"].tensor.numpy()
            finally:
                np.random.choice = real_choice
            out[name + "_next_uniform"] = np.array(np.random.uniform(), np.float64)
            remove = kw["remove_close"]
            if available is None:
                order = np.zeros(0, np.int64)
                copies = SWEEPS_NUM if kw["pad_empty_sweeps"] else 0
                key_removed = key0[~((np.abs(key0[:, 0]) < 1.0) & (np.abs(key0[:, 1]) < 1.0))]
                want = np.concatenate([key0] + [key_removed] * copies, 0)
                out["key_removed"] = key_removed
                assert 0 < len(key_removed) < len(key0)
            else:
                order = chosen[0] if chosen else np.arange(min(available, SWEEPS_NUM))
                assert len(chosen) == (1 if available > SWEEPS_NUM and not kw.get("test_mode") else 0)
                rows, at = [key0], len(key0)
                for i in order:  # cut the reference's output into its sweeps: each must be the ordered float64 restatement
                    mine = restate(sweeps[i], l2s[i], TIMESTAMP - stamps[i], remove)
                    piece = got[at:at + len(mine)][:, :LOAD_DIM] if kw["use_dim"] == FULL else mine
                    at += len(mine)
                    store = pieces if remove else raw_pieces
                    if kw["use_dim"] == FULL:
                        assert piece.shape == mine.shape and np.array_equal(_bits(piece), _bits(mine)), (name, int(i))
                        assert i not in store or np.array_equal(_bits(store[i]), _bits(piece))
                        store[i] = piece.copy()
                    rows.append(mine)
                    if remove:
                        assert 0 < len(mine) < len(sweeps[i]), "sweep %d loses %d rows of %d" % (i, len(sweeps[i]) - len(mine), len(sweeps[i]))
                want = np.concatenate(rows, 0)
            want = want[:, kw["use_dim"]]
            assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), name
            orders.append(np.asarray(order, np.int64))
            out[name + "_choices"] = orders[-1]
            out[name + "_seed"] = np.array(seed)
            out[name + "_available"] = np.array(-1 if available is None else available)
            out[name + "_use_dim"] = np.array(kw["use_dim"])
            out[name + "_flags"] = np.array([kw["pad_empty_sweeps"], kw["remove_close"], kw.get("test_mode", False)])
            print("%-10s %5d rows, choices %s" % (name, len(got), orders[-1].tolist()))
    train = [tuple(out["train%d_choices" % d].tolist()) for d in range(3)]
    assert len(set(train)) == 3 and all(list(c) != sorted(c) for c in train), train
    assert sorted(pieces) == list(range(N_SWEEPS)), "some sweep was never chosen -- choose other seeds"
    for i in range(N_SWEEPS):
        out["piece%d" % i] = pieces[i]
    for i, p in raw_pieces.items():
        out["raw_piece%d" % i] = p
    values = sum(p[:, :3].size for p in pieces.values()) + sum(p[:, :3].size for p in raw_pieces.values())
    print("coordinates held to the ordered float64 restatement bit for bit:", values)
    path = os.path.join(HERE, "multi_sweep.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
