"""CPU: ObjectSample + DataBaseSampler against the reference's recorded draws (tests/golden/object_sample.npz), the collision
test's known answers, the paste step of the plan and the LiDAR config's train pipeline built by name."""
import pickle

import numpy as np
import pytest
import torch

import object_sample_cases as cases
from bevfusion_amd import object_sample as osm
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor
from bevfusion_amd.registry import TRANSFORMS

RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]


@pytest.fixture(scope="module")
def cfg(tmp_path_factory):
    return cases.write_database(tmp_path_factory.mktemp("object_sample_db"))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def test_builds_by_name_with_the_reference_keywords(cfg):
    t = TRANSFORMS.build(dict(type="ObjectSample", db_sampler=dict(cfg)))
    assert isinstance(t, osm.ObjectSample) and isinstance(t.db_sampler, osm.DataBaseSampler)
    assert t.disabled is False and t.sample_2d is False and t.use_ground_plane is False and t.defer is False
    s = TRANSFORMS.build(dict(type="DataBaseSampler", **cfg))
    g = cases.golden()
    # `prepare` took out the object with too few points and the one of a removed difficulty
    kept = int(((g["db_num_points_in_gt"] >= int(g["min_points"])) & (g["db_difficulty"] != -1)).sum())
    assert sum(len(v) for v in s.db_infos.values()) == kept < len(g["db_class"])
    assert s.sample_classes == [str(n) for n in g["group_names"]] and s.sample_max_nums == [int(n) for n in g["group_nums"]]


@pytest.mark.parametrize("arrays", [False, True])
def test_golden_draws_boxes_labels_points_and_generator_calls(cfg, arrays):
    g = cases.golden()
    n_gt = len(g["gt_boxes"])
    for d in range(cases.n_draws()):
        outs, nxt = cases.run(cfg, d, arrays=arrays)
        for c, data in enumerate(outs):
            boxes, labels, points = cases.reference(d, c)
            kind = np.ndarray if arrays else torch.Tensor
            assert isinstance(data["points"], kind) and isinstance(data["gt_bboxes_3d"], kind)
            got_boxes, got_labels = np.asarray(data["gt_bboxes_3d"]), np.asarray(data["gt_labels_3d"])
            assert got_labels.dtype == np.int64 and got_boxes.dtype == np.float32
            assert np.array_equal(_bits(got_boxes[:n_gt]), _bits(g["gt_boxes"])) and np.array_equal(got_labels[:n_gt], g["gt_labels"])
            assert np.array_equal(_bits(got_boxes[n_gt:]), _bits(boxes)), (d, c)
            assert np.array_equal(got_labels[n_gt:], labels), (d, c)
            got = np.asarray(data["points"])
            assert got.dtype == np.float32 and got.shape == points.shape and np.array_equal(_bits(got), _bits(points)), (d, c)
        assert nxt == float(g["draw%d_next_uniform" % d]), d  # the reference's generator calls, no more and no fewer


def test_plane_mask_is_the_reference_mask(cfg):
    g = cases.golden()
    pts = torch.from_numpy(g["points"])
    for d in range(cases.n_draws()):
        for c in range(cases.n_calls()):
            planes = pa.paste_planes(g["draw%d_call%d_boxes" % (d, c)])
            assert planes.dtype == np.float32 and planes.shape == (len(g["draw%d_call%d_boxes" % (d, c)]), 6, 4)
            mask = pa.points_in_any_box(pts, torch.from_numpy(planes)).numpy()
            assert np.array_equal(mask, g["draw%d_call%d_mask" % (d, c)]), (d, c)


def test_eager_and_deferred_give_the_same_rows(cfg):
    for d in (0, 3):
        eager, nxt_e = cases.run(cfg, d)
        deferred, nxt_d = cases.run(cfg, d, defer=True)
        assert nxt_e == nxt_d
        for e, x in zip(eager, deferred):
            assert torch.equal(x["points"], torch.from_numpy(cases.golden()["points"]))  # untouched
            plan = x["points_aug_plan"]
            assert plan.paste_points is not None and plan.paste_planes.shape[1:] == (6, 4) and plan.stage == 0
            assert np.array_equal(_bits(pa.torch_points_aug(x["points"], plan)), _bits(e["points"]))
            assert torch.equal(x["gt_bboxes_3d"], e["gt_bboxes_3d"]) and np.array_equal(x["gt_labels_3d"], e["gt_labels_3d"])


def _bev(boxes):
    b = np.asarray(boxes, np.float32)
    return pa.box_corners(b[:, 0:2], b[:, 3:5], b[:, 6], 0.5)


def _off_diagonal(coll):
    """A box against itself has collinear edges and corners on its own edges: that entry hangs on rounding, and the sampler
    clears the diagonal as the reference does."""
    coll = coll.copy()
    coll[np.arange(len(coll)), np.arange(len(coll))] = False
    return coll


def test_collision_known_answers():
    big = [0, 0, 0, 4, 4, 1, 0.3]
    inside = [0.2, 0.1, 0, 1, 1, 1, 1.0]      # wholly inside `big`: no edges cross, only the complete-overlap checks see it
    crossing = [1, 0, 0, 4, 1, 1, 1.2]
    disjoint = [20, 0, 0, 2, 2, 1, 0.5]
    c = _bev([big, inside, crossing, disjoint])
    want = np.array([[0, 1, 1, 0], [1, 0, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0]], bool)
    assert np.array_equal(_off_diagonal(osm.box_collision_test(c, c)), want)
    # a box that only touches another along an edge (the hulls share a side: zero overlap) is free, axis-aligned ...
    c = _bev([[0, 0, 0, 4, 4, 1, 0.0], [4, 0, 0, 4, 4, 1, 0.0], [4.5, 0.5, 0, 4, 4, 1, 0.0]])
    assert np.array_equal(_off_diagonal(osm.box_collision_test(c, c)), np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0]], bool))
    # ... and boxes whose hulls overlap but which do not meet are free too
    c = _bev([[0, 0, 0, 6, 1, 1, np.pi / 4], [2.5, -2.5, 0, 1, 1, 1, 0.0]])
    assert not _off_diagonal(osm.box_collision_test(c, c)).any()


def test_sampler_drops_a_sample_inside_a_ground_truth_box(cfg):
    np.random.seed(0)
    s = TRANSFORMS.build(dict(type="DataBaseSampler", **cfg))
    name = s.sample_classes[0]
    first = s.sampler_dict[name]._sampled_list[s.sampler_dict[name]._indices[0]]["box3d_lidar"]
    around = first.copy()
    around[3:5] = 3 * first[3:5]  # a ground-truth box that holds the first object the class's sampler will hand out
    valid = s.sample_class_v2(name, 2, around[None])
    assert len(valid) <= 1 and all(not np.array_equal(v["box3d_lidar"], first) for v in valid)


def test_disabled_is_a_no_op_without_generator_calls(cfg):
    t = TRANSFORMS.build(dict(type="ObjectSample", db_sampler=dict(cfg), defer=True))
    t.disabled = True  # what DisableObjectSampleHook does
    np.random.seed(5)
    want = np.random.uniform()
    np.random.seed(5)
    data = cases.frame()
    before = {k: (v.clone() if torch.is_tensor(v) else v.copy()) for k, v in data.items()}
    out = t.transform(data)
    assert np.random.uniform() == want
    assert set(out) == set(before) and all(np.array_equal(np.asarray(out[k]), np.asarray(before[k])) for k in before)


def test_sample_2d_raises(cfg):
    with pytest.raises(NotImplementedError):
        TRANSFORMS.build(dict(type="ObjectSample", db_sampler=dict(cfg), sample_2d=True))


def test_ground_plane_lowers_boxes_and_points(cfg):
    plane = np.array([0.0, 0.0, 1.0, 0.25])  # dz = z + 0.25
    np.random.seed(1)
    a = TRANSFORMS.build(dict(type="DataBaseSampler", **cfg)).sample_all(cases.golden()["gt_boxes"], cases.golden()["gt_labels"])
    np.random.seed(1)
    b = TRANSFORMS.build(dict(type="DataBaseSampler", **cfg)).sample_all(cases.golden()["gt_boxes"], cases.golden()["gt_labels"],
                                                                         ground_plane=plane)
    dz = a["gt_bboxes_3d"][:, 2].astype(np.float64) + 0.25
    assert np.allclose(b["gt_bboxes_3d"][:, 2], a["gt_bboxes_3d"][:, 2] - dz, atol=1e-6)
    assert np.array_equal(b["gt_bboxes_3d"][:, [0, 1, 3, 4, 5, 6]], a["gt_bboxes_3d"][:, [0, 1, 3, 4, 5, 6]])
    assert torch.equal(a["points"][:, [0, 1, 3, 4]], b["points"][:, [0, 1, 3, 4]]) and not torch.equal(a["points"][:, 2], b["points"][:, 2])
    with pytest.raises(ValueError):
        TRANSFORMS.build(dict(type="ObjectSample", db_sampler=dict(cfg), use_ground_plane=True)).transform(cases.frame())


def test_paste_must_be_the_first_step_and_the_plan_pickles(cfg):
    g = cases.golden()
    boxes, pasted = g["draw0_call0_boxes"], g["draw0_call0_pasted"]
    for first in (lambda p: p.set_rts(np.eye(3), [0, 0, 0], 1.0, "RTS"), lambda p: p.set_flip(1, 0), lambda p: p.set_range(RANGE),
                  lambda p: p.set_shuffle(1), lambda p: p.set_paste(pasted, boxes)):
        with pytest.raises(ValueError):
            first(pa.PointsAugPlan()).set_paste(pasted, boxes)
    plan = pa.PointsAugPlan().set_paste(pasted, boxes).set_rts(np.eye(3), [0.5, 0, 0], 1.1, "RST").set_range(RANGE).set_shuffle(9)
    back = pickle.loads(pickle.dumps(plan))
    for key in pa.PointsAugPlan.__slots__:
        a, b = getattr(plan, key), getattr(back, key)
        assert np.array_equal(a, b) and type(a) is type(b), key
    pts = torch.from_numpy(g["points"])
    assert torch.equal(pa.torch_points_aug(pts, back), pa.torch_points_aug(pts, plan))
    # a plan without a paste pickles as it did before the paste existed: no paste keys in its state
    plain = pa.PointsAugPlan().set_range(RANGE)
    assert set(plain.__getstate__()) == {"rot", "trans", "scale", "order", "flip_horizontal", "flip_vertical", "range", "shuffle",
                                         "seed", "stage"}
    assert pickle.loads(pickle.dumps(plain)).paste_points is None
    with pytest.raises(ValueError):  # pasted rows of another width than the cloud
        pa.torch_points_aug(pts, pa.PointsAugPlan().set_paste(pasted[:, :4], boxes))


def test_deferred_paste_refuses_point_masks(cfg):
    t = TRANSFORMS.build(dict(type="ObjectSample", db_sampler=dict(cfg), defer=True))
    data = cases.frame()
    data["pts_semantic_mask"] = np.zeros(len(data["points"]), np.int64)
    with pytest.raises(ValueError):
        t.transform(data)


def _lidar_train_pipeline(cfg, defer, shuffle):
    """The reference LiDAR config's train_pipeline between LoadAnnotations3D and Pack3DDetInputs."""
    extra = dict(defer=True) if defer else {}
    steps = [dict(type="GlobalRotScaleTrans", scale_ratio_range=[0.9, 1.1], rot_range=[-0.78539816, 0.78539816], translation_std=0.5,
                  **extra),
             dict(type="BEVFusionRandomFlip3D", **extra), dict(type="PointsRangeFilter", point_cloud_range=RANGE, **extra),
             dict(type="ObjectRangeFilter", point_cloud_range=RANGE), dict(type="ObjectNameFilter", classes=cfg["classes"])]
    return steps + ([dict(type="PointShuffle", **extra)] if shuffle else [])


def test_lidar_config_train_pipeline_builds_by_name_and_runs_deferred(cfg):
    eager, nxt_e = cases.run(cfg, 2, after=_lidar_train_pipeline(cfg, False, False))
    deferred, nxt_d = cases.run(cfg, 2, defer=True, after=_lidar_train_pipeline(cfg, True, False))
    assert nxt_e == nxt_d
    pre = Det3DDataPreprocessor()
    before = dict(pa.PATHS)
    out = pre(dict(inputs=dict(points=[x["points"] for x in deferred], points_aug_plan=[x["points_aug_plan"] for x in deferred])))
    assert pa.PATHS["torch"] == before["torch"] + 1 and pa.PATHS["kernel"] == before["kernel"]
    for got, e, x in zip(out["inputs"]["points"], eager, deferred):
        assert 0 < len(got) and np.array_equal(_bits(got), _bits(e["points"]))
        assert torch.equal(x["gt_bboxes_3d"], e["gt_bboxes_3d"]) and np.array_equal(x["gt_labels_3d"], e["gt_labels_3d"])
        assert len(x["gt_labels_3d"]) > len(cases.golden()["gt_labels"]) - 3  # pasted boxes came through the object filters
    # with the shuffle: the same rows in another order
    torch.manual_seed(4)
    shuffled, _ = cases.run(cfg, 2, defer=True, after=_lidar_train_pipeline(cfg, True, True))
    got = pre.process_points([x["points"] for x in shuffled], [x["points_aug_plan"] for x in shuffled])
    for s, e in zip(got, eager):
        a, b = s.numpy(), np.asarray(e["points"])
        assert a.shape == b.shape and not np.array_equal(a, b)
        assert np.array_equal(a[np.lexsort(a.T)], b[np.lexsort(b.T)])
