"""Shared by tests/test_points_aug_cpu.py and tests/test_points_aug_gpu.py: the recorded reference draws
(tests/golden/points_aug.npz, written by tests/golden/make_points_aug_golden.py), this package's chain on the same inputs and
the tolerance between two float32 evaluations of the chain.

The tolerance is derived, not measured.  Per coordinate the chain is a three-term float32 dot product with |r| <= 1, one add and
one multiply.  Two evaluations of the dot product (any order, fused or not) differ by at most 2 gamma_3 (|x| + |y| + |z|),
gamma_3 = 3u / (1 - 3u), u = 2^-24; the add and the multiply that follow each round once on either side.  With the magnitudes
bounded by s (|x| + |y| + |z| + |t_c|) that is below 12 * 2^-24 * s * (|x| + |y| + |z| + |t_c|)."""
import os

import numpy as np
import torch

from bevfusion_amd import points_aug as pa
from bevfusion_amd.registry import TRANSFORMS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_aug.npz")
GRST = dict(rot_range=[-0.78539816, 0.78539816], scale_ratio_range=[0.9, 1.1], translation_std=[0.5, 0.5, 0.5])
U12 = 12.0 * 2.0 ** -24

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def n_draws():
    return int(golden()["n_draws"])


def kind(d):
    return str(golden()["draw%d_kind" % d])


def draw_of(k):
    """The first draw of kind k."""
    return [kind(d) for d in range(n_draws())].index(k)


def pipeline(d, defer=False, shuffle=False):
    """The transforms of draw d's chain, built by name."""
    g = golden()
    rng = [float(v) for v in g["point_cloud_range"]]
    k = kind(d)
    extra = dict(defer=True) if defer else {}
    steps = []
    if k != "test":
        steps.append(dict(type="GlobalRotScaleTrans" if k == "plain" else "BEVFusionGlobalRotScaleTrans", **GRST, **extra))
        steps.append(dict(type="BEVFusionRandomFlip3D", **extra))
    steps.append(dict(type="PointsRangeFilter", point_cloud_range=rng, **extra))
    if k in ("bev", "plain"):
        steps.append(dict(type="ObjectRangeFilter", point_cloud_range=rng))
        steps.append(dict(type="ObjectNameFilter", classes=["class%d" % i for i in range(int(g["n_classes"]))]))
    if shuffle:
        steps.append(dict(type="PointShuffle", **extra))
    return [TRANSFORMS.build(s) for s in steps]


def run(d, defer=False, shuffle=False, arrays=False):
    """Draw d through this package's chain under the draw's seed -> (data, the next np.random.uniform())."""
    g = golden()
    pts, boxes, labels = g["points"].copy(), g["boxes"].copy(), g["labels"].copy()
    data = dict(points=pts if arrays else torch.from_numpy(pts))
    if kind(d) in ("bev", "plain"):
        data["gt_bboxes_3d"] = boxes if arrays else torch.from_numpy(boxes)
        data["gt_labels_3d"] = labels
    np.random.seed(int(g["draw%d_seed" % d]))
    for t in pipeline(d, defer, shuffle):
        data = t.transform(data)
    return data, np.random.uniform()


def tolerance(d, xyz=None, trans=None):
    """[n, 3] float64: the bound for draw d on the rows `xyz` (default: the fixture's points) with translation `trans`."""
    g = golden()
    xyz = g["points"][:, :3] if xyz is None else xyz
    trans = g["draw%d_trans" % d] if trans is None else trans
    mag = np.abs(np.asarray(xyz, np.float64)).sum(1, keepdims=True) + np.abs(np.asarray(trans, np.float64))[None, :]
    return U12 * float(g["draw%d_scale" % d]) * mag


def reference_points(d):
    """float32 [kept, C]: what the reference's chain left of the points, before the shuffle."""
    g = golden()
    mask = g["draw%d_mask" % d]
    return np.concatenate([g["draw%d_xyz" % d], g["points"][mask][:, 3:]], 1)


def assert_points_match(d, ours):
    """ours [kept, C] (filtered, unshuffled) against the reference: same rows kept, xyz within the bound, the rest equal."""
    g = golden()
    ref, mask = reference_points(d), g["draw%d_mask" % d]
    ours = np.asarray(ours)
    assert ours.dtype == np.float32 and ours.shape == ref.shape, (ours.shape, ref.shape)
    assert np.array_equal(ours[:, 3:], ref[:, 3:])  # the untouched columns identify the rows: the kept mask is identical
    err = np.abs(ours[:, :3].astype(np.float64) - ref[:, :3].astype(np.float64))
    tol = tolerance(d)[mask]
    print("draw %d: max |ours - ref| / bound = %.3f" % (d, float((err / tol).max())))
    assert (err <= tol).all()


def full_plan(d, shuffle=False):
    """The PointsAugPlan the deferred chain writes for draw d."""
    data, _ = run(d, defer=True, shuffle=shuffle)
    return data["points_aug_plan"]
