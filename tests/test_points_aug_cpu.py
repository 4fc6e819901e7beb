"""CPU: the LiDAR augmentation chain (bevfusion_amd/points_aug.py) against the reference's recorded draws
(tests/golden/points_aug.npz), the deferred plan, the shuffle bijection and the preprocessor's torch path."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import points_aug_cases as cases
from bevfusion_amd import _lib
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor
from bevfusion_amd.registry import MODELS, TRANSFORMS

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DRAWS = list(range(cases.n_draws()))
NAMES = ("BEVFusionGlobalRotScaleTrans", "GlobalRotScaleTrans", "BEVFusionRandomFlip3D", "PointsRangeFilter",
         "ObjectRangeFilter", "ObjectNameFilter", "PointShuffle")


def test_fixture_covers_every_case():
    g = cases.golden()
    kinds = [cases.kind(d) for d in DRAWS]
    assert kinds.count("bev") >= 4 and {"plain", "noboxes", "test"} <= set(kinds)
    flips = {tuple(int(v) for v in g["draw%d_flips" % d]) for d in DRAWS if cases.kind(d) == "bev"}
    assert flips == {(0, 0), (0, 1), (1, 0), (1, 1)}
    n = len(g["points"])
    assert all(0.3 * n < g["draw%d_mask" % d].sum() < 0.8 * n for d in DRAWS)
    assert len(g["draw0_boxes"]) < len(g["boxes"])  # some boxes leave


@pytest.mark.parametrize("arrays", [False, True])
@pytest.mark.parametrize("d", DRAWS)
def test_sampler_matrix_and_boxes(d, arrays):
    g = cases.golden()
    data, nxt = cases.run(d, arrays=arrays)
    k = cases.kind(d)
    assert nxt == float(g["draw%d_next_uniform" % d])  # the same number of generator calls
    if k == "test":
        assert "lidar_aug_matrix" not in data and "transformation_3d_flow" not in data
        return
    assert np.array_equal(np.float64(data["pcd_rotation_angle"]), g["draw%d_angle" % d])
    assert np.array_equal(np.float64(data["pcd_scale_factor"]), g["draw%d_scale" % d])
    assert data["pcd_trans"].dtype == np.float64 and np.array_equal(data["pcd_trans"], g["draw%d_trans" % d])
    assert data["pcd_rotation"].dtype == torch.float32 and np.array_equal(data["pcd_rotation"].numpy(), g["draw%d_rotation" % d])
    assert [int(data["pcd_horizontal_flip"]), int(data["pcd_vertical_flip"])] == g["draw%d_flips" % d].tolist()
    assert data["lidar_aug_matrix"].dtype == np.float64 and np.array_equal(data["lidar_aug_matrix"], g["draw%d_matrix" % d])
    assert "".join(data["transformation_3d_flow"]) == str(g["draw%d_flow" % d]) == ("RST" if k == "plain" else "RTS")
    if k == "noboxes":
        return
    boxes, labels = data["gt_bboxes_3d"], data["gt_labels_3d"]
    assert isinstance(boxes, np.ndarray) == arrays
    boxes = np.asarray(boxes)
    want = g["draw%d_boxes" % d]
    assert np.array_equal(np.asarray(labels), g["draw%d_labels" % d])
    assert boxes.shape == want.shape and boxes.dtype == np.float32
    # which input rows survived, from the reference's record: sizes scale exactly (one multiply), so they identify the row
    s32 = np.float32(g["draw%d_scale" % d])
    src = [int(np.flatnonzero((g["boxes"][:, 3:6] * s32 == w[3:6]).all(1))[0]) for w in want]
    assert src == sorted(set(src))  # distinct input rows, in their order: identical rows kept
    assert np.array_equal(boxes[:, 3:6], want[:, 3:6])
    src_boxes = g["boxes"][src]
    angle = float(g["draw%d_angle" % d])
    err = np.abs(boxes.astype(np.float64) - want.astype(np.float64))
    assert (err[:, :3] <= cases.tolerance(d, src_boxes[:, :3])).all()
    vel = np.concatenate([src_boxes[:, 7:9], np.zeros((len(src), 1), np.float32)], 1)
    assert (err[:, 7:9] <= cases.tolerance(d, vel, np.zeros(3))[:, :2]).all()
    # the yaw: the same float32 scalar operations on either side (add, negate, + pi, the period wrap)
    assert (err[:, 6] <= cases.U12 * (np.abs(src_boxes[:, 6]) + abs(angle) + 3 * np.pi)).all()
    assert (np.abs(boxes[:, 6]) <= np.pi + 1e-6).all()


@pytest.mark.parametrize("d", DRAWS)
def test_points_against_the_reference(d):
    data, _ = cases.run(d)
    assert torch.is_tensor(data["points"])
    cases.assert_points_match(d, data["points"].numpy())
    arr, _ = cases.run(d, arrays=True)
    assert isinstance(arr["points"], np.ndarray) and np.array_equal(arr["points"], data["points"].numpy())


@pytest.mark.parametrize("d", DRAWS)
def test_deferred_plan_gives_the_eager_bits_and_the_reference_mask(d):
    g = cases.golden()
    eager, _ = cases.run(d)
    deferred, nxt = cases.run(d, defer=True)
    assert nxt == float(g["draw%d_next_uniform" % d])
    assert np.array_equal(deferred["points"].numpy(), g["points"])  # untouched
    plan = deferred["points_aug_plan"]
    out, mask = pa.torch_points_aug(deferred["points"], plan, return_mask=True)
    assert np.array_equal(mask.numpy(), g["draw%d_mask" % d])
    assert torch.equal(out, eager["points"])
    for key in ("lidar_aug_matrix", "gt_bboxes_3d", "gt_labels_3d", "pcd_trans"):
        if key in eager:
            assert np.array_equal(np.asarray(eager[key]), np.asarray(deferred[key])), key


def test_registry_builds_all_seven_by_name():
    g = cases.golden()
    rng = [float(v) for v in g["point_cloud_range"]]
    cfgs = dict(BEVFusionGlobalRotScaleTrans=cases.GRST, GlobalRotScaleTrans=cases.GRST, BEVFusionRandomFlip3D={},
                PointsRangeFilter=dict(point_cloud_range=rng), ObjectRangeFilter=dict(point_cloud_range=rng),
                ObjectNameFilter=dict(classes=["car"]), PointShuffle={})
    assert set(cfgs) == set(NAMES)
    for name in NAMES:
        t = TRANSFORMS.build(dict(type=name, **cfgs[name]))
        assert type(t) is getattr(pa, name) and name not in MODELS
    for name in ("BEVFusionGlobalRotScaleTrans", "GlobalRotScaleTrans", "BEVFusionRandomFlip3D", "PointsRangeFilter", "PointShuffle"):
        assert TRANSFORMS.build(dict(type=name, defer=True, **cfgs[name])).defer


def test_plan_is_small_and_survives_pickle():
    torch.manual_seed(3)
    plan = cases.full_plan(0, shuffle=True)
    assert plan.order == "RTS" and plan.range is not None and plan.shuffle and 0 <= plan.seed < 2 ** 64
    assert plan.rot.dtype == plan.trans.dtype == plan.range.dtype == np.float32 and isinstance(plan.scale, np.float32)
    blob = pickle.dumps(plan)
    assert len(blob) < 2048
    back = pickle.loads(blob)
    for key in pa.PointsAugPlan.__slots__:
        a, b = getattr(plan, key), getattr(back, key)
        assert np.array_equal(a, b) and type(a) is type(b), key
    pts = torch.from_numpy(cases.golden()["points"])
    assert torch.equal(pa.torch_points_aug(pts, plan), pa.torch_points_aug(pts, back))
    assert cases.full_plan(cases.draw_of("plain")).order == "RST" and cases.full_plan(cases.draw_of("test")).order is None


def test_deferred_shuffle_draws_one_seed_from_torchs_generator():
    torch.manual_seed(11)
    plan = cases.full_plan(0, shuffle=True)
    after = torch.rand(1)
    torch.manual_seed(11)
    want = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    assert plan.seed == want and torch.equal(after, torch.rand(1))


def test_unsupported_deferred_cases_raise():
    g = cases.golden()
    rng = [float(v) for v in g["point_cloud_range"]]
    pts = torch.from_numpy(g["points"].copy())
    with pytest.raises(ValueError, match="shift_height"):
        pa.GlobalRotScaleTrans(shift_height=True, defer=True)
    for key in ("pts_instance_mask", "pts_semantic_mask"):
        with pytest.raises(ValueError, match=key):
            pa.PointsRangeFilter(rng, defer=True).transform({"points": pts, key: np.zeros(len(pts), np.int64)})
    # orders the plan cannot express
    data = pa.PointsRangeFilter(rng, defer=True).transform(dict(points=pts))
    with pytest.raises(ValueError, match="cannot follow"):
        pa.BEVFusionRandomFlip3D(defer=True).transform(data)
    data = pa.PointShuffle(defer=True).transform(dict(points=pts))
    with pytest.raises(ValueError, match="cannot follow"):
        pa.PointsRangeFilter(rng, defer=True).transform(data)
    data = pa.BEVFusionGlobalRotScaleTrans(defer=True, **cases.GRST).transform(dict(points=pts))
    with pytest.raises(ValueError, match="cannot follow"):
        pa.GlobalRotScaleTrans(defer=True, **cases.GRST).transform(data)
    data = pa.PointsRangeFilter(rng, defer=True).transform(dict(points=pts))
    with pytest.raises(ValueError, match="cannot follow"):
        pa.PointsRangeFilter(rng, defer=True).transform(data)
    with pytest.raises(ValueError):
        pa.torch_points_aug(torch.zeros(4, 2), pa.PointsAugPlan())


def test_eager_shuffle_is_randperm():
    pts = torch.from_numpy(cases.golden()["points"].copy())
    torch.manual_seed(5)
    out = pa.PointShuffle().transform(dict(points=pts.clone()))["points"]
    torch.manual_seed(5)
    assert torch.equal(out, pts[torch.randperm(len(pts))])
    torch.manual_seed(5)
    inst = np.arange(len(pts))
    both = pa.PointShuffle().transform(dict(points=pts.numpy().copy(), pts_instance_mask=inst))
    assert np.array_equal(both["points"], out.numpy()) and np.array_equal(pts.numpy()[both["pts_instance_mask"]], out.numpy())


@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 1000, 1024])
def test_deferred_shuffle_is_a_permutation(n):
    rows = torch.arange(n * 4, dtype=torch.float32).view(n, 4)
    plans = [pa.PointsAugPlan().set_shuffle(seed) for seed in (7, 7, 8)]
    a, b, c = (pa.torch_points_aug(rows, p) for p in plans)
    assert a.shape == rows.shape and torch.equal(a[a[:, 0].argsort()], rows)  # a permutation of the rows
    assert torch.equal(a, b)
    if n >= 64:
        assert not torch.equal(a, c) and not torch.equal(a, rows)
    perm = pa.shuffle_permutation(7, n)
    assert perm.dtype == torch.int64 and torch.equal(perm.sort().values, torch.arange(n))
    assert torch.equal(a[perm], rows)  # output row perm(r) holds the r-th row


def test_deferred_shuffle_follows_the_filter():
    torch.manual_seed(2)
    plan = cases.full_plan(2, shuffle=True)
    pts = torch.from_numpy(cases.golden()["points"])
    out = pa.torch_points_aug(pts, plan)
    plan.shuffle = False
    plain = pa.torch_points_aug(pts, plan)
    perm = pa.shuffle_permutation(plan.seed, len(plain))
    assert torch.equal(out[perm], plain) and not torch.equal(out, plain)


def test_every_order_of_five_occurs_among_20000_consecutive_seeds():
    perms = pa.shuffle_permutations(range(20000), 5)
    assert torch.equal(perms.sort(1).values, torch.arange(5).repeat(20000, 1))
    codes = (perms * torch.tensor([625, 125, 25, 5, 1])).sum(1)
    assert len(codes.unique()) == 120
    assert torch.equal(perms[123], pa.shuffle_permutation(123, 5))


def test_shuffle_keys_are_32_bit_and_seed_dependent():
    a, b = pa.shuffle_keys(0), pa.shuffle_keys(1)
    assert len(a) == pa.ROUNDS == 6 and all(0 <= k < 2 ** 32 for k in a + b) and a != b
    assert pa.shuffle_keys(2 ** 64 + 5) == pa.shuffle_keys(5)


def test_preprocessor_on_cpu_equals_the_eager_transforms():
    draws = [0, 2, cases.draw_of("plain"), cases.draw_of("noboxes"), cases.draw_of("test")]
    eager = [cases.run(d)[0]["points"] for d in draws]
    deferred = [cases.run(d, defer=True)[0] for d in draws]
    pre = Det3DDataPreprocessor()
    before = dict(pa.PATHS)
    out = pre(dict(inputs=dict(points=[x["points"] for x in deferred], points_aug_plan=[x["points_aug_plan"] for x in deferred])))
    got = out["inputs"]["points"]
    assert pa.PATHS["torch"] == before["torch"] + 1 and pa.PATHS["kernel"] == before["kernel"]
    assert len(got) == len(draws) and all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(got, eager))
    base = got[0].untyped_storage().data_ptr()
    assert all(t.untyped_storage().data_ptr() == base for t in got)  # views of one buffer
    assert "points_aug_plan" not in out["inputs"]
    # float64 and non-contiguous points: the same bits
    wide = torch.from_numpy(np.concatenate([cases.golden()["points"]] * 2, 1))[:, :5]
    assert not wide.is_contiguous()
    got = pre.process_points([deferred[0]["points"].double(), wide], [deferred[0]["points_aug_plan"]] * 2)
    assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[0])
    with pytest.raises(ValueError, match="plans for"):
        pre.process_points([wide], [])


def test_preprocessor_with_a_shuffle_and_without_a_plan():
    torch.manual_seed(9)
    deferred = cases.run(3, defer=True, shuffle=True)[0]
    eager = cases.run(3)[0]["points"]
    pre = Det3DDataPreprocessor()
    got = pre(dict(inputs=dict(points=[deferred["points"]], points_aug_plan=[deferred["points_aug_plan"]])))["inputs"]["points"][0]
    assert got.shape == eager.shape and not torch.equal(got, eager)
    key = lambda t: t[np.lexsort(t.numpy().T[::-1])]  # noqa: E731
    assert torch.equal(key(got), key(eager))  # the eager rows in another order
    pts = [torch.from_numpy(cases.golden()["points"])]
    out = pre(dict(inputs=dict(points=pts)))["inputs"]["points"]
    assert out[0] is pts[0]  # no plan: points pass through as before


def test_descriptor_layout_matches_the_header(tmp_path):
    import subprocess
    fields = [name for name, _ in pa._Sample._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bevfusion_hip.h"\nint main(void) {\n'
                   '  printf("%zu %d", sizeof(bfhip_points_aug_sample), BFHIP_POINTS_AUG_ROUNDS);\n' +
                   "".join('  printf(" %%zu", offsetof(bfhip_points_aug_sample, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(pa._Sample), pa.ROUNDS] + [getattr(pa._Sample, f).offset for f in fields]


def test_entry_point_rejects_bad_arguments_before_any_launch():
    """Host-side checks only: every call here returns before a launch."""
    lib = _lib.load()
    block = lib.bfhip_points_aug_block()
    assert block >= 64 and block % 64 == 0
    assert _lib.call_size("bfhip_points_aug_workspace_bytes", 1000, 2) >= ((1000 + block - 1) // block + 2) * 4
    kept = (ctypes.c_int32 * 2)()
    fake = 4096  # never dereferenced

    def call(descs, n, C, out=fake, work=fake, work_bytes=1 << 20):
        _lib.call("bfhip_points_aug", descs, n, C, out, kept, work, work_bytes, None)

    descs = (pa._Sample * 2)()
    descs[0].points, descs[0].n, descs[1].points, descs[1].n = fake, 1000, fake, 10
    for C in (2, 9):
        with pytest.raises(RuntimeError, match="columns"):
            call(descs, 2, C)
    with pytest.raises(RuntimeError, match="n_samples"):
        call(descs, 0, 5)
    with pytest.raises(RuntimeError, match="workspace"):
        call(descs, 2, 5, work_bytes=8)
    with pytest.raises(RuntimeError, match="out is NULL"):
        call(descs, 2, 5, out=None)
    descs[1].flags = 64
    with pytest.raises(RuntimeError, match="flags"):
        call(descs, 2, 5)
    descs[1].flags, descs[1].n = 0, -1
    with pytest.raises(RuntimeError, match="n=-1"):
        call(descs, 2, 5)
    descs[1].n, descs[1].points = 10, None
    with pytest.raises(RuntimeError, match="sample 1"):
        call(descs, 2, 5)
    descs[1].points = fake + 2
    with pytest.raises(RuntimeError, match="aligned"):
        call(descs, 2, 5)
    descs[0].n, descs[1].n, descs[1].points = 2 ** 31 - 1, 1, fake
    with pytest.raises(RuntimeError, match="2\\^31"):
        call(descs, 2, 5)
    assert not pa.fused_supported([torch.zeros(4, 5)]) and not pa.fused_supported([])


def test_paste_and_sweeps_entries_reject_bad_arguments_before_any_launch():
    """Host-side checks only, through the driver the three entries share: every call here returns before a launch.  The cases
    are those of test_object_sample_gpu.py::test_invalid_arguments_are_rejected and of test_multi_sweep_gpu.py::
    test_invalid_tables_are_rejected_and_nothing_is_launched, without their valid calls."""
    lib = _lib.load()
    kept = (ctypes.c_int32 * 1)()
    fake = 4096  # never dereferenced
    descs = (pa._Sample * 1)()
    descs[0].points, descs[0].n = fake, 8

    def paste(points=fake, n_points=8, planes=fake + 128, n_boxes=2, pastes=True, C=4, out=fake, bytes_=1 << 20, n_samples=1):
        p = (pa._Paste * 1)()
        p[0].points, p[0].n_points, p[0].planes, p[0].n_boxes = points, n_points, planes, n_boxes
        return lib.bfhip_points_aug_paste(descs, p if pastes else None, n_samples, C, out, kept, fake, bytes_, None)

    def sweeps(first=(0, 4, 8), n_segments=2, segments=fake, pastes=None, sweeps=True, C=5, out=fake, bytes_=1 << 20, n_samples=1):
        w = (pa._Sweeps * 1)()
        w[0].segments, w[0].n_segments = segments, n_segments
        w[0].first[:len(first)] = list(first)
        return lib.bfhip_points_aug_sweeps(descs, pastes, w if sweeps else None, n_samples, C, out, kept, fake, bytes_, None)

    def rejected(entry, text, **kw):
        assert entry(**kw) == -1, kw  # BFHIP_E_INVALID
        msg = lib.bfhip_last_error().decode()
        assert msg.startswith("points_aug_%s: " % entry.__name__) and text in msg, (kw, msg)

    rejected(paste, "n_boxes=65 (0 .. 64)", n_boxes=65)
    rejected(paste, "n_boxes=-1", n_boxes=-1)
    rejected(paste, "n_points=-1", n_points=-1)
    rejected(paste, "n_points=8 points=", points=None)
    rejected(paste, "n_boxes=2 (0 .. 64) planes=", planes=None)
    rejected(paste, "a required pointer is NULL", pastes=False)
    rejected(paste, "not 4-byte aligned", points=fake + 2)
    rejected(paste, "not 4-byte aligned", planes=fake + 1)
    rejected(paste, "2 columns (3 .. 8)", C=2)
    rejected(paste, "9 columns (3 .. 8)", C=9)
    rejected(paste, "n_samples=0", n_samples=0)
    rejected(paste, "out is NULL", out=None)
    rejected(paste, "workspace of 0 bytes", bytes_=0)

    rejected(sweeps, "boundary 2 (8) is below boundary 1 (9)", first=(0, 9, 8))
    rejected(sweeps, "boundaries run from 0 to 7", first=(0, 4, 7))
    rejected(sweeps, "boundaries run from 1 to 8", first=(1, 4, 8))
    rejected(sweeps, "n_segments=17 (0 .. 16)", n_segments=17)
    rejected(sweeps, "n_segments=-1", n_segments=-1)
    rejected(sweeps, "n_segments=2 (0 .. 16) segments=", segments=None)
    rejected(sweeps, "4 columns (5 .. 8", C=4)
    rejected(sweeps, "4 columns (5 .. 8", C=4, n_segments=0, segments=None)  # even without a sweep step
    rejected(sweeps, "9 columns (5 .. 8", C=9)
    rejected(sweeps, "segments not 8-byte aligned", segments=fake + 4)
    rejected(sweeps, "a required pointer is NULL", sweeps=False)
    rejected(sweeps, "n_samples=0", n_samples=0)
    rejected(sweeps, "out is NULL", out=None)
    rejected(sweeps, "workspace of 0 bytes", bytes_=0)
    # the sweeps entry with paste descriptors: the same paste checks, and the pasted rows count towards the 2^31 bound
    p = (pa._Paste * 1)()
    p[0].points, p[0].n_points, p[0].planes, p[0].n_boxes = fake, 8, fake + 128, 65
    rejected(sweeps, "n_boxes=65 (0 .. 64)", pastes=p)
    p[0].n_boxes, p[0].n_points = 2, 2 ** 31 - 8
    rejected(sweeps, "2^31", pastes=p)
    rejected(paste, "2^31", n_points=2 ** 31 - 8)


def test_eager_shift_height_scales_the_named_column():
    pts = cases.golden()["points"].copy()
    np.random.seed(4)
    plain = pa.GlobalRotScaleTrans(**cases.GRST).transform(dict(points=pts.copy()))
    np.random.seed(4)
    shifted = pa.GlobalRotScaleTrans(shift_height=True, **cases.GRST).transform(dict(points=pts.copy(), points_height_dim=3))
    s32 = np.float32(plain["pcd_scale_factor"])
    assert np.array_equal(shifted["points"][:, [0, 1, 2, 4]], plain["points"][:, [0, 1, 2, 4]])
    assert np.array_equal(shifted["points"][:, 3], plain["points"][:, 3] * s32)
    with pytest.raises(ValueError, match="points_height_dim"):
        pa.GlobalRotScaleTrans(shift_height=True, **cases.GRST).transform(dict(points=pts.copy()))
