"""CPU: LoadPointsFromFile + LoadPointsFromMultiSweeps against the reference's recorded runs (tests/golden/multi_sweep.npz), the
sweep step of the plan, and the nuScenes configs' LiDAR pipelines built by name from the first step to the last."""
import pickle

import numpy as np
import pytest
import torch

import multi_sweep_cases as cases
import object_sample_cases as os_cases
from bevfusion_amd import loading
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor
from bevfusion_amd.registry import TRANSFORMS

RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
FULL = [n for n in cases.names() if n != "usedim"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return cases.write_files(tmp_path_factory.mktemp("multi_sweep"))


@pytest.fixture(scope="module")
def db(tmp_path_factory):
    return os_cases.write_database(tmp_path_factory.mktemp("multi_sweep_db"))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def test_the_fixture_covers_its_cases():
    g = cases.golden()
    assert set(cases.names()) == {"train0", "train1", "train2", "test", "few", "none_pad", "none_nopad", "noremove", "usedim"}
    assert len(g["sweep_counts"]) == 12 and int(g["sweeps_num"]) == 9 and int(g["load_dim"]) == 5
    assert list(g["test_choices"]) == list(range(9)) and list(g["few_choices"]) == [0, 1, 2, 3]
    assert len({tuple(g["train%d_choices" % d]) for d in range(3)}) == 3
    starts = np.concatenate([[0], np.cumsum(g["sweep_counts"])])
    for i in range(12):  # every sweep: rows inside the square go, rows exactly on its border stay
        raw = g["sweep_points"][starts[i]:starts[i + 1]]
        inside = (np.abs(raw[:, 0]) < 1.0) & (np.abs(raw[:, 1]) < 1.0)
        border = ((np.abs(raw[:, 0]) == 1.0) & (np.abs(raw[:, 1]) <= 1.0)) | ((np.abs(raw[:, 1]) == 1.0) & (np.abs(raw[:, 0]) <= 1.0))
        assert inside.sum() > 0 and border.sum() >= 6 and not (inside & border).any()
        assert len(g["piece%d" % i]) == len(raw) - inside.sum()


@pytest.mark.parametrize("tensor", [False, True])
@pytest.mark.parametrize("name", cases.names())
def test_eager_transforms_equal_the_reference_bit_for_bit(files, name, tensor):
    data, nxt = cases.run(files, name, tensor=tensor)
    assert isinstance(data["points"], torch.Tensor if tensor else np.ndarray)
    assert _same(data["points"], cases.reference(name)), name
    assert nxt == float(cases.golden()[name + "_next_uniform"])  # the reference's generator calls, no more and no fewer
    assert "points_aug_plan" not in data


@pytest.mark.parametrize("name", FULL)
def test_deferred_plan_through_torch_points_aug_equals_the_reference(files, name):
    g = cases.golden()
    data, nxt = cases.run(files, name, defer=True)
    assert nxt == float(g[name + "_next_uniform"])
    plan, pts = data["points_aug_plan"], data["points"]
    assert isinstance(pts, np.ndarray) and pts.dtype == np.float32 and pts.flags["C_CONTIGUOUS"]
    # untouched file contents: the keyframe, then the chosen sweeps' raw rows
    starts = np.concatenate([[0], np.cumsum(g["sweep_counts"])])
    raw = [g["keyframe"]] + [g["sweep_points"][starts[i]:starts[i + 1]] for i in g[name + "_choices"]]
    if name == "none_pad":
        raw = [g["keyframe"]] * 10
    assert np.array_equal(_bits(pts), _bits(np.concatenate(raw, 0)))
    assert list(plan.sweep_starts) == list(np.concatenate([[0], np.cumsum([len(r) for r in raw])]))
    assert plan.stage == 0 and plan.sweep_dt.dtype == np.float32 and len(plan.sweep_dt) == len(raw) - 1
    if name == "none_pad":
        assert plan.sweep_l2s is None and not plan.sweep_dt.any() and plan.sweep_remove
    elif len(raw) > 1:
        assert plan.sweep_l2s.dtype == np.float64 and plan.sweep_l2s.shape == (len(raw) - 1, 4, 4)
        want_dt = np.float32(float(g["timestamp"]) - g["sweep_timestamps"][g[name + "_choices"]])
        assert np.array_equal(plan.sweep_dt, want_dt)
    assert _same(pa.torch_points_aug(pts, plan).numpy(), cases.reference(name))


def test_keywords_defaults_and_unsupported_values():
    t = TRANSFORMS.build(dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=5, use_dim=5, backend_args=dict(x=1)))
    assert type(t) is loading.LoadPointsFromFile and t.use_dim == [0, 1, 2, 3, 4]
    m = TRANSFORMS.build(dict(type="LoadPointsFromMultiSweeps"))
    assert type(m) is loading.LoadPointsFromMultiSweeps
    assert (m.sweeps_num, m.load_dim, m.use_dim, m.pad_empty_sweeps, m.remove_close, m.test_mode, m.defer) == \
        (10, 5, [0, 1, 2, 4], False, False, False, False)
    for key in ("shift_height", "use_color", "norm_intensity", "norm_elongation"):
        with pytest.raises(NotImplementedError):
            loading.LoadPointsFromFile("LIDAR", **{key: True})
    with pytest.raises(ValueError):
        loading.LoadPointsFromFile("LIDAR", load_dim=4, use_dim=[0, 1, 2, 4])
    with pytest.raises(ValueError, match="defer=False"):
        loading.LoadPointsFromMultiSweeps(use_dim=[0, 1, 2, 4], defer=True)
    with pytest.raises(ValueError, match="defer=False"):
        loading.LoadPointsFromMultiSweeps(load_dim=9, use_dim=9, defer=True)
    assert loading.LoadPointsFromMultiSweeps(load_dim=6, use_dim=6, defer=True).defer


def test_load_points_from_file_takes_use_dim(files):
    g = cases.golden()
    t = loading.LoadPointsFromFile("LIDAR", load_dim=5, use_dim=[0, 1, 2, 4])
    out = t.transform(dict(lidar_points=dict(lidar_path=files[0])))["points"]
    assert _same(out, g["keyframe"][:, [0, 1, 2, 4]])


def _plan_with_sweeps():
    l2s = cases.golden()["lidar2sensor"][:2]
    return pa.PointsAugPlan().set_sweeps([0, 5, 8, 12], l2s, [0.05, 0.1], True)


def test_sweep_step_order_in_the_plan():
    g = cases.golden()
    paste, boxes = os_cases.golden()["draw0_call0_pasted"], os_cases.golden()["draw0_call0_boxes"]
    plan = _plan_with_sweeps().set_paste(paste, boxes).set_rts(np.eye(3), [0, 0, 0], 1.0, "RTS").set_range(RANGE)  # accepted
    assert plan.sweep_starts is not None and plan.paste_points is not None and plan.stage == 3
    with pytest.raises(ValueError):  # a second one
        _plan_with_sweeps().set_sweeps([0, 5, 8, 12], g["lidar2sensor"][:2], [0.05, 0.1], True)
    for first in (lambda p: p.set_paste(paste, boxes), lambda p: p.set_rts(np.eye(3), [0, 0, 0], 1.0, "RTS"), lambda p: p.set_flip(1, 0),
                  lambda p: p.set_range(RANGE), lambda p: p.set_shuffle(1)):
        with pytest.raises(ValueError, match="defer=False"):  # after any other step
            first(pa.PointsAugPlan()).set_sweeps([0, 5, 8, 12], g["lidar2sensor"][:2], [0.05, 0.1], True)
    for bad in ([0, 5, 8], [1, 5, 8, 12], [0, 9, 8, 12]):  # too few boundaries, not from 0, decreasing
        with pytest.raises(ValueError):
            pa.PointsAugPlan().set_sweeps(bad, g["lidar2sensor"][:2], [0.05, 0.1], True)
    with pytest.raises(ValueError):  # the cloud's rows are not the plan's
        pa.torch_points_aug(torch.zeros(11, 5), _plan_with_sweeps())
    with pytest.raises(ValueError):  # no column for the time lag
        pa.torch_points_aug(torch.zeros(12, 4), _plan_with_sweeps())


def test_plan_with_sweeps_pickles_and_one_without_is_as_before(files):
    data, _ = cases.run(files, "train1", defer=True, after=[dict(type="PointsRangeFilter", point_cloud_range=RANGE, defer=True)])
    plan = data["points_aug_plan"]
    back = pickle.loads(pickle.dumps(plan))
    for key in pa.PointsAugPlan.__slots__:
        a, b = getattr(plan, key), getattr(back, key)
        assert np.array_equal(a, b) and type(a) is type(b), key
    assert back.sweep_l2s.dtype == np.float64 and back.sweep_starts.dtype == np.int64
    assert torch.equal(pa.torch_points_aug(data["points"], back), pa.torch_points_aug(data["points"], plan))
    plain = pa.PointsAugPlan().set_range(RANGE)
    assert set(plain.__getstate__()) == {"rot", "trans", "scale", "order", "flip_horizontal", "flip_vertical", "range", "shuffle",
                                         "seed", "stage"}
    assert pickle.loads(pickle.dumps(plain)).sweep_starts is None


def test_segment_table_is_the_c_struct():
    plan = _plan_with_sweeps()
    seg = pa.sweep_segments(plan)
    assert pa.SEGMENT.itemsize == 112 and seg.shape == (3,) and [pa.SEGMENT.fields[k][1] for k in ("first", "flags", "dt", "radius", "m", "t")] == \
        [0, 4, 8, 12, 16, 88]
    assert list(seg["first"]) == [0, 5, 8] and list(seg["flags"]) == [0, 3, 3] and list(seg["dt"]) == [0, np.float32(0.05), np.float32(0.1)]
    assert np.array_equal(seg["m"][1].reshape(3, 3), plan.sweep_l2s[0, :3, :3]) and np.array_equal(seg["t"][2], plan.sweep_l2s[1, :3, 3])
    assert (seg["radius"] == 1.0).all()
    padded = pa.PointsAugPlan().set_sweeps([0, 5, 8], None, [0.0], True)
    assert list(pa.sweep_segments(padded)["flags"]) == [0, 1]


def test_synthetic_sample_through_both_modes(tmp_path):
    from bevfusion_amd import synthetic
    s = synthetic.multi_sweep_sample(seed=5, key_rows=700, sweep_rows=300, sweeps=3)
    again = synthetic.multi_sweep_sample(seed=5, key_rows=700, sweep_rows=300, sweeps=3)
    assert all(np.array_equal(a, b) for a, b in zip(s["sweeps"], again["sweeps"])) and np.array_equal(s["lidar2sensor"], again["lidar2sensor"])
    assert s["keyframe"].shape == (700, 5) and s["keyframe"].dtype == np.float32 and len(s["sweeps"]) == 3
    rot = s["lidar2sensor"][:, :3, :3]
    assert np.allclose(rot @ rot.transpose(0, 2, 1), np.eye(3), atol=1e-12) and np.allclose(np.linalg.det(rot), 1.0)  # rigid
    infos = []
    for i, p in enumerate(s["sweeps"]):
        close = (np.abs(p[:, 0]) < 1) & (np.abs(p[:, 1]) < 1)
        assert 0 < close.sum() < len(p) and ((np.abs(p[:, 0]) == 1) | (np.abs(p[:, 1]) == 1)).any()
        p.tofile(str(tmp_path / ("s%d.bin" % i)))
        infos.append(dict(lidar_points=dict(lidar_path=str(tmp_path / ("s%d.bin" % i)), lidar2sensor=s["lidar2sensor"][i]),
                          timestamp=s["sweep_timestamps"][i]))
    outs = []
    for defer in (False, True):
        t = loading.LoadPointsFromMultiSweeps(sweeps_num=9, use_dim=5, remove_close=True, defer=defer)
        outs.append(t.transform(dict(points=s["keyframe"].copy(), timestamp=s["timestamp"], lidar_sweeps=infos)))
    eager, deferred = outs
    assert len(deferred["points"]) == 700 + sum(len(p) for p in s["sweeps"]) > len(eager["points"]) > 700
    assert _same(pa.torch_points_aug(deferred["points"], deferred["points_aug_plan"]).numpy(), eager["points"])
    lag = np.float32(s["timestamp"] - s["sweep_timestamps"])
    assert set(eager["points"][700:, 4].tolist()) == set(lag.tolist()) and (eager["points"][:700, 4] == 0).all()


def _pipeline(db, defer, train, shuffle=True):
    """The LiDAR steps of the nuScenes configs' train_pipeline / test_pipeline, in their order (LoadAnnotations3D and
    Pack3DDetInputs aside); the reference's keywords."""
    extra = dict(defer=True) if defer else {}
    load = [dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=5, use_dim=5, backend_args=None),
            dict(type="LoadPointsFromMultiSweeps", sweeps_num=9, load_dim=5, use_dim=5, pad_empty_sweeps=True, remove_close=True,
                 backend_args=None, test_mode=not train, **extra)]
    if not train:
        return load + [dict(type="PointsRangeFilter", point_cloud_range=RANGE, **extra)]
    return load + [dict(type="ObjectSample", db_sampler=dict(db), **extra),
                   dict(type="GlobalRotScaleTrans", scale_ratio_range=[0.9, 1.1], rot_range=[-0.78539816, 0.78539816],
                        translation_std=0.5, **extra),
                   dict(type="BEVFusionRandomFlip3D", **extra), dict(type="PointsRangeFilter", point_cloud_range=RANGE, **extra),
                   dict(type="ObjectRangeFilter", point_cloud_range=RANGE), dict(type="ObjectNameFilter", classes=db["classes"])] + \
        ([dict(type="PointShuffle", **extra)] if shuffle else [])


def _run_pipeline(files, db, defer, train, shuffle=True, seed=7):
    np.random.seed(seed)
    torch.manual_seed(seed)
    steps = [TRANSFORMS.build(s) for s in _pipeline(db, defer, train, shuffle)]
    data = cases.frame(files, "train0")
    if train:  # what LoadAnnotations3D adds
        og = os_cases.golden()
        data.update(gt_bboxes_3d=og["gt_boxes"].copy(), gt_labels_3d=og["gt_labels"].copy())
    for t in steps:
        data = t.transform(data)
    return data, np.random.uniform()


@pytest.mark.parametrize("train", [True, False])
def test_nuscenes_pipelines_build_by_name_and_deferred_equals_eager(files, db, train):
    eager, nxt_e = _run_pipeline(files, db, False, train, shuffle=False)
    deferred, nxt_d = _run_pipeline(files, db, True, train, shuffle=False)
    assert nxt_e == nxt_d
    plan = deferred["points_aug_plan"]
    assert plan.sweep_starts is not None and plan.range is not None and (plan.paste_points is not None) == train
    before = dict(pa.PATHS)
    out = Det3DDataPreprocessor()(dict(inputs=dict(points=[torch.from_numpy(deferred["points"])], points_aug_plan=[plan])))
    assert pa.PATHS["torch"] == before["torch"] + 1 and pa.PATHS["kernel"] == before["kernel"]
    got = out["inputs"]["points"][0]
    assert 1000 < len(got) < len(deferred["points"]) and _same(got.numpy(), eager["points"])
    if train:
        assert np.array_equal(deferred["gt_bboxes_3d"], eager["gt_bboxes_3d"])
        shuffled, _ = _run_pipeline(files, db, True, True, shuffle=True)  # with the shuffle: the same rows in another order
        a = pa.torch_points_aug(shuffled["points"], shuffled["points_aug_plan"]).numpy()
        b = np.asarray(eager["points"])
        assert a.shape == b.shape and not np.array_equal(_bits(a), _bits(b))
        assert np.array_equal(_bits(a[np.lexsort(_bits(a).T)]), _bits(b[np.lexsort(_bits(b).T)]))
