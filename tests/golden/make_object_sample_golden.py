#!/usr/bin/env python3
"""Writes tests/golden/object_sample.npz: the reference's own ObjectSample + DataBaseSampler on a small synthetic database and
a seeded frame, for tests/test_object_sample_cpu.py and tests/test_object_sample_gpu.py.

The reference's classes are loaded at run time from REFERENCE_ROOT (default /root/reference) behind stubs of the packages that
are not installed (as make_points_aug_golden.py does); nothing of it is copied.  Real files: mmdet3d/utils/array_converter.py,
structures/bbox_3d/utils.py, structures/points/{base,lidar}_points.py, structures/bbox_3d/{base,lidar}_box3d.py,
structures/ops/box_np_ops.py, datasets/transforms/{data_augment_utils,dbsampler,transforms_3d}.py.  mmengine's file helpers
are stubbed with pickle, LoadPointsFromFile with np.fromfile, and numba with an identity jit / njit.

Under the identity jit `box_collision_test`'s `ret[i, j] is True` / `is False` tests are never true for numpy bools, so its
complete-overlap branch never runs and a box wholly inside another reads as free, which compiled numba does not do.  The
database and ground-truth boxes are therefore drawn such that no box holds all four corners of another (`contains`, an
independent check in float64, asserted over every pair), and both executions decide alike.

Inputs: a database of N_CLASSES classes x N_OBJECTS objects (20-60 points each, 5 floats per point; a few more objects that
`prepare` must filter out), a cloud of N_POINTS points [n, 5], most of them scattered around database boxes so that pasted boxes
hold some, and N_GT ground-truth boxes.  Draws: per seed, np.random.seed(seed), the transform is built (the samplers shuffle)
and called CALLS times on the same frame, so the class indices wrap and reshuffle; after the calls the next
np.random.uniform() is recorded.  Per call: the sampled boxes and labels, the sampled points, the mask of removed points; the
output points are [sampled points ; points[~mask]] (asserted).

Asserted as well: some call rejects a sample by collision; some call pastes three or more classes; every call removes between
2 % and 50 % of the points; every plane sign of every (point, database box, plane) is further from zero than 4 * 2^-24 * (|x n0|
+ |y n1| + |z n2| + |d|), the rounding bound of the four-term float32 sum, so any evaluation order gives the same mask (points
of the seeded cloud that violate this are taken out of the input before anything is recorded)."""
import contextlib
import importlib.util
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
N_POINTS, N_GT, N_CLASSES, N_OBJECTS, LOAD_DIM, CALLS = 2000, 8, 6, 6, 5, 3
CLASSES = ["class%d" % i for i in range(N_CLASSES)]
SAMPLE_GROUPS = dict(class0=3, class1=2, class2=4, class3=2, class4=3, class5=2)
MIN_POINTS = 5
SEEDS = (0, 1, 2, 3, 4)


class _Any(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (object,), {})


class _Registry:
    def __init__(self):
        self.modules = {}

    def register_module(self, *a, **k):
        def _do(cls):
            self.modules[cls.__name__] = cls
            return cls
        return _do

    def build(self, cfg):
        cfg = dict(cfg)
        return self.modules[cfg.pop("type")](**cfg)


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


def _jit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda fn: fn


class _Logger:
    @classmethod
    def get_current_instance(cls):
        return cls()

    def info(self, *a, **k):
        pass


def load_reference():
    for name in ("cv2", "mmcv", "mmcv.transforms", "mmcv.ops", "mmdet", "mmdet.datasets", "mmdet.datasets.transforms",
                 "mmdet3d", "mmdet3d.models", "mmdet3d.models.task_modules", "mmdet3d.structures", "mmdet3d.structures.ops",
                 "mmdet3d.structures.bbox_3d", "mmdet3d.datasets", "mmdet3d.datasets.transforms", "numba.core"):
        _stub(name)
    _stub("numba", jit=_jit, njit=_jit)
    _stub("numba.core.errors", NumbaPerformanceWarning=type("NumbaPerformanceWarning", (Warning,), {}))
    _stub("mmengine", load=lambda f, file_format=None: pickle.load(f))
    _stub("mmengine.fileio", get_local_path=lambda path, backend_args=None: contextlib.nullcontext(path))
    _stub("mmengine.logging", MMLogger=_Logger)
    registry = _Registry()
    _stub("mmdet3d.registry", TRANSFORMS=registry)
    ac = _load("mmdet3d.utils.array_converter", "mmdet3d/utils/array_converter.py")
    _stub("mmdet3d.utils", array_converter=ac.array_converter)
    ut = _load("mmdet3d.structures.bbox_3d.utils", "mmdet3d/structures/bbox_3d/utils.py")
    for name in ("limit_period", "points_cam2img", "rotation_3d_in_axis"):
        setattr(sys.modules["mmdet3d.structures.bbox_3d"], name, getattr(ut, name))
    bp = _load("mmdet3d.structures.points.base_points", "mmdet3d/structures/points/base_points.py")
    lp = _load("mmdet3d.structures.points.lidar_points", "mmdet3d/structures/points/lidar_points.py")
    _stub("mmdet3d.structures.points", BasePoints=bp.BasePoints, LiDARPoints=lp.LiDARPoints)
    _load("mmdet3d.structures.bbox_3d.base_box3d", "mmdet3d/structures/bbox_3d/base_box3d.py")
    lb = _load("mmdet3d.structures.bbox_3d.lidar_box3d", "mmdet3d/structures/bbox_3d/lidar_box3d.py")
    sys.modules["mmdet3d.structures"].LiDARInstance3DBoxes = lb.LiDARInstance3DBoxes
    sys.modules["mmdet3d.structures"].BasePoints = bp.BasePoints
    ops = _load("mmdet3d.structures.ops.box_np_ops", "mmdet3d/structures/ops/box_np_ops.py")
    sys.modules["mmdet3d.structures.ops"].box_np_ops = ops
    dau = _load("mmdet3d.datasets.transforms.data_augment_utils", "mmdet3d/datasets/transforms/data_augment_utils.py")
    sys.modules["mmdet3d.datasets.transforms"].data_augment_utils = dau
    _load("mmdet3d.datasets.transforms.dbsampler", "mmdet3d/datasets/transforms/dbsampler.py")
    t3 = _load("mmdet3d.datasets.transforms.transforms_3d", "mmdet3d/datasets/transforms/transforms_3d.py")

    class LoadPointsFromFile:  # what the sampler's points_loader needs of it
        def __init__(self, coord_type, load_dim, use_dim, backend_args=None):
            self.load_dim, self.use_dim = load_dim, list(range(use_dim)) if isinstance(use_dim, int) else use_dim

        def __call__(self, results):
            pts = np.fromfile(results["lidar_points"]["lidar_path"], dtype=np.float32).reshape(-1, self.load_dim)[:, self.use_dim]
            results["points"] = lp.LiDARPoints(pts, points_dim=pts.shape[-1])
            return results

    registry.modules["LoadPointsFromFile"] = LoadPointsFromFile
    return lp.LiDARPoints, lb.LiDARInstance3DBoxes, ops, t3


def corners_bev(box):
    """float64 [4, 2]: the bird's-eye-view corners of one box."""
    c, s = np.cos(float(box[6])), np.sin(float(box[6]))
    half = np.array([[-1, -1], [-1, 1], [1, 1], [1, -1]], np.float64) * np.array([box[3], box[4]], np.float64) / 2
    return half @ np.array([[c, s], [-s, c]]) + np.array([box[0], box[1]], np.float64)


def contains(outer, inner, slack=1e-3):
    """Does `outer` hold all four corners of `inner` (bird's-eye view, float64, with some slack)?"""
    c, s = np.cos(float(outer[6])), np.sin(float(outer[6]))
    local = (corners_bev(inner) - np.array([outer[0], outer[1]], np.float64)) @ np.array([[c, -s], [s, c]])
    return bool((np.abs(local[:, 0]) <= outer[3] / 2 + slack).all() and (np.abs(local[:, 1]) <= outer[4] / 2 + slack).all())


def make_boxes(rs, n, taken):
    """n boxes [n, 7] float32 over +-30 m, none holding or held by one of `taken` or of themselves."""
    out = []
    while len(out) < n:
        b = np.array([rs.uniform(-30, 30), rs.uniform(-30, 30), rs.uniform(-2.0, -1.0), rs.uniform(3.4, 4.6), rs.uniform(1.6, 2.2),
                      rs.uniform(1.4, 2.0), rs.uniform(-np.pi, np.pi)]).astype(np.float32)
        if not any(contains(o, b) or contains(b, o) for o in list(taken) + out):
            out.append(b)
    return np.stack(out)


def make_inputs():
    rs = np.random.RandomState(17)
    gt = make_boxes(rs, N_GT, [])
    gt_labels = rs.randint(0, N_CLASSES, N_GT).astype(np.int64)
    db_boxes = make_boxes(rs, N_CLASSES * N_OBJECTS, gt).reshape(N_CLASSES, N_OBJECTS, 7)
    objects = []  # (class, box, points relative to the centre, num_points_in_gt, difficulty)
    for c in range(N_CLASSES):
        for o in range(N_OBJECTS):
            box = db_boxes[c, o]
            n = int(rs.randint(20, 61))
            p = ((rs.rand(n, LOAD_DIM) - 0.5) * np.array([box[3], box[4], box[5], 1, 1])).astype(np.float32)
            p[:, 2] += box[5] / 2  # above the bottom centre
            objects.append((c, box, p, n, 0))
    for c, n, difficulty in ((1, 3, 0), (4, 30, -1)):  # what `prepare` must take out: too few points, removed difficulty
        box = db_boxes[c, 0].copy()
        objects.append((c, box, np.zeros((n, LOAD_DIM), np.float32), n, difficulty))
    centres = db_boxes.reshape(-1, 7)
    near = centres[rs.randint(0, len(centres), int(0.7 * N_POINTS))]
    clustered = np.concatenate([near[:, :2] + rs.normal(scale=1.3, size=(len(near), 2)), rs.uniform(-3, 1.5, (len(near), 1))], 1)
    spread = np.concatenate([rs.uniform(-50, 50, (N_POINTS - len(near), 2)), rs.uniform(-3, 1.5, (N_POINTS - len(near), 1))], 1)
    xyz = np.concatenate([clustered, spread], 0)[rs.permutation(N_POINTS)]
    pts = np.concatenate([xyz, rs.rand(N_POINTS, 2)], 1).astype(np.float32)
    return pts, gt, gt_labels, objects


def planes_of(ops, boxes):
    """(normal [K, 6, 3], d [K, 6]) as points_in_rbbox computes them."""
    corners = ops.center_to_corner_box3d(boxes[:, :3], boxes[:, 3:6], boxes[:, 6], origin=(0.5, 0.5, 0), axis=2)
    return ops.surface_equ_3d(ops.corner_to_surfaces_3d(corners)[:, :, :3, :])


def margins_ok(ops, pts, boxes):
    """bool [n]: every plane sign of the point further from zero than the rounding bound of the four-term float32 sum."""
    normal, d = planes_of(ops, boxes)
    terms = pts[:, None, None, :3].astype(np.float64) * normal[None].astype(np.float64)  # [n, K, 6, 3]
    sign = terms.sum(-1) + d[None].astype(np.float64)
    bound = 4.0 * 2.0 ** -24 * (np.abs(terms).sum(-1) + np.abs(d[None].astype(np.float64)))
    return (np.abs(sign) > bound).all((1, 2))


def write_database(root, objects):
    infos = {name: [] for name in CLASSES}
    for i, (c, box, p, n, difficulty) in enumerate(objects):
        rel = "db/%d_%s.bin" % (i, CLASSES[c])
        os.makedirs(os.path.join(root, "db"), exist_ok=True)
        p.tofile(os.path.join(root, rel))
        infos[CLASSES[c]].append(dict(name=CLASSES[c], path=rel, box3d_lidar=box.copy(), num_points_in_gt=n, difficulty=difficulty,
                                      image_idx=0, gt_idx=i, group_id=i))
    path = os.path.join(root, "dbinfos.pkl")
    with open(path, "wb") as f:
        pickle.dump(infos, f)
    return path


def sampler_cfg(root, info_path):
    return dict(data_root=root, info_path=info_path, rate=1.0,
                prepare=dict(filter_by_difficulty=[-1], filter_by_min_points={name: MIN_POINTS for name in CLASSES}),
                classes=CLASSES, sample_groups=dict(SAMPLE_GROUPS),
                points_loader=dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=LOAD_DIM, use_dim=list(range(LOAD_DIM))))


def main():
    LiDARPoints, Boxes, ops, t3 = load_reference()
    pts, gt, gt_labels, objects = make_inputs()
    every_box = np.concatenate([gt] + [o[1][None] for o in objects], 0)
    for i, a in enumerate(every_box[:N_GT + N_CLASSES * N_OBJECTS]):
        for j, b in enumerate(every_box[:N_GT + N_CLASSES * N_OBJECTS]):
            assert i == j or not contains(a, b, slack=0.0), "box %d holds box %d" % (i, j)
    db_boxes = np.stack([o[1] for o in objects[:N_CLASSES * N_OBJECTS]])
    ok = margins_ok(ops, pts, db_boxes)
    print("points within the rounding bound of a plane, taken out:", int((~ok).sum()))
    pts = np.ascontiguousarray(pts[ok])

    out = dict(points=pts, gt_boxes=gt, gt_labels=gt_labels, load_dim=np.array(LOAD_DIM), min_points=np.array(MIN_POINTS),
               classes=np.array(CLASSES), group_names=np.array(list(SAMPLE_GROUPS)), group_nums=np.array(list(SAMPLE_GROUPS.values())),
               db_class=np.array([o[0] for o in objects]), db_boxes=np.stack([o[1] for o in objects]),
               db_points=np.concatenate([o[2] for o in objects], 0), db_counts=np.array([len(o[2]) for o in objects]),
               db_num_points_in_gt=np.array([o[3] for o in objects]), db_difficulty=np.array([o[4] for o in objects]),
               seeds=np.array(SEEDS), calls=np.array(CALLS))
    rejected = many_classes = False
    with tempfile.TemporaryDirectory() as root:
        info_path = write_database(root, objects)
        for d, seed in enumerate(SEEDS):
            np.random.seed(seed)
            transform = t3.ObjectSample(db_sampler=sampler_cfg(root, info_path))
            sampler, drawn = transform.db_sampler, []
            for batch_sampler in sampler.sampler_dict.values():  # how many objects each class's sampler hands out ...
                batch_sampler.sample = lambda num, inner=batch_sampler.sample: drawn.append(inner(num)) or drawn[-1]
            inner_v2 = sampler.sample_class_v2

            def sample_class_v2(name, num, avoid):  # ... against how many the collision test lets through
                nonlocal rejected
                valid = inner_v2(name, num, avoid)
                rejected |= len(valid) < len(drawn[-1])
                return valid

            sampler.sample_class_v2 = sample_class_v2
            for c in range(CALLS):
                data = dict(points=LiDARPoints(torch.from_numpy(pts.copy()), points_dim=LOAD_DIM),
                            gt_bboxes_3d=Boxes(torch.from_numpy(gt.copy()), box_dim=7), gt_labels_3d=gt_labels.copy())
                data = transform.transform(data)
                boxes = data["gt_bboxes_3d"].tensor.numpy()[N_GT:]
                labels = data["gt_labels_3d"][N_GT:]
                assert data["gt_labels_3d"].dtype == np.int64 and np.array_equal(data["gt_bboxes_3d"].tensor.numpy()[:N_GT], gt)
                wanted = sum(max(0, num - int((gt_labels == CLASSES.index(name)).sum())) for name, num in SAMPLE_GROUPS.items())
                many_classes |= len(set(labels.tolist())) >= 3
                assert margins_ok(ops, pts, boxes).all()
                mask = ops.points_in_rbbox(pts, boxes).any(-1)
                assert 0.02 * len(pts) < mask.sum() < 0.5 * len(pts), (d, c, int(mask.sum()))
                result = data["points"].tensor.numpy()
                m = len(result) - int((~mask).sum())
                assert m > 0 and np.array_equal(result[m:], pts[~mask])
                print("draw %d call %d: %d boxes of %d wanted, %d pasted points, %d points removed"
                      % (d, c, len(boxes), wanted, m, int(mask.sum())))
                key = "draw%d_call%d_" % (d, c)
                out[key + "boxes"], out[key + "labels"], out[key + "pasted"], out[key + "mask"] = boxes, labels, result[:m], mask
            out["draw%d_next_uniform" % d] = np.array(np.random.uniform(), np.float64)
    assert rejected, "no call rejected a sample by collision -- choose other seeds"
    assert many_classes, "no call pasted three or more classes -- choose other seeds"
    path = os.path.join(HERE, "object_sample.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
