"""CPU: GridMask (bevfusion_amd/image_aug.py) -- the host class against the reference's recorded draws (tests/golden/grid_mask.npz,
written by tests/golden/make_grid_mask_golden.py), `torch_grid_mask` against PIL itself, the deferred record on the plan and
the preprocessor's torch path.  The mask is integer work and the frames are multiplied by 0 or 1: every comparison is exact."""
import copy
import json
import os
import pickle

import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
import points_aug_cases
from bevfusion_amd import image_aug as ia
from bevfusion_amd import synthetic
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor
from bevfusion_amd.registry import MODELS, TRANSFORMS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_mask.npz")
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
SHIPPED = dict(type="GridMask", use_h=True, use_w=True, max_epoch=6, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.0,
               fixed_prob=True)  # the camera + LiDAR config's own


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def cases(g):
    for i in range(int(g["n_cases"])):
        c = {k: g["case%d_%s" % (i, k)] for k in ("set", "cfg", "seed", "epoch", "applied", "ints", "mask", "out", "next_uniform")}
        c["cfg"] = json.loads(str(c["cfg"]))
        c["frames"] = g["frames_" + str(c["set"])].astype(np.float32)
        yield i, c


def build(c, **extra):
    aug = TRANSFORMS.build(dict(type="GridMask", **c["cfg"], **extra))
    if int(c["epoch"]) >= 0:
        aug.set_epoch(int(c["epoch"]))
    return aug


def test_registered_with_the_reference_keywords_and_defaults():
    assert TRANSFORMS.get("GridMask") is ia.GridMask and "GridMask" not in MODELS
    aug = TRANSFORMS.build(dict(type="GridMask", use_h=True, use_w=False, max_epoch=6))
    assert (aug.rotate, aug.offset, aug.ratio, aug.mode, aug.prob, aug.st_prob, aug.fixed_prob, aug.defer) == \
        (1, False, 0.5, 0, 1.0, 1.0, False, False)
    aug.set_epoch(3)
    assert aug.prob == 0.5 and aug.epoch == 3
    fixed = TRANSFORMS.build(dict(SHIPPED, prob=0.7))
    fixed.set_epoch(3)
    assert fixed.prob == 0.7


def test_golden_holds_what_the_tests_need(golden):
    """A skipped and an applied draw at prob 0.6 and at the epoch's 0.5, every parameter value, r = 0 and a quarter turn on the
    square frames (the generator asserts the fill pixels and the row beyond the last band from the reference alone)."""
    all_cases = [c for _, c in cases(golden)]
    for prob in (0.6, 1.0):
        at = [bool(c["applied"]) for c in all_cases if c["cfg"]["prob"] == prob and (prob == 0.6 or not c["cfg"]["fixed_prob"])]
        assert True in at and False in at, prob
    applied = [c for c in all_cases if c["applied"]]
    assert {c["cfg"]["mode"] for c in applied} == {0, 1} and {c["cfg"]["ratio"] for c in applied} == {0.5, 1}
    assert {(c["cfg"]["use_h"], c["cfg"]["use_w"]) for c in applied} == {(True, False), (False, True), (True, True)}
    square = {int(c["ints"][4]) for c in applied if str(c["set"]) == "b" and c["cfg"]["rotate"] == 360}
    assert 0 in square and square & {90, 180, 270}
    assert any(c["mask"].min() == 0 and c["mask"].max() == 1 for c in applied)


def test_host_class_reproduces_every_recorded_draw(golden):
    for i, c in cases(golden):
        aug = build(c)
        frames = [f.copy() for f in c["frames"]]
        np.random.seed(int(c["seed"]))
        out = aug.transform(dict(img=frames))
        assert np.random.uniform() == float(c["next_uniform"]), "case %d leaves the generator in another state" % i
        got = np.stack(out["img"])
        assert got.dtype == np.float32 and np.array_equal(got, c["out"].astype(np.float32)), "case %d frames" % i
        if not c["applied"]:
            assert all(a is b for a, b in zip(out["img"], frames))  # untouched
            continue
        h, w = c["frames"].shape[1:3]
        np.random.seed(int(c["seed"]))
        np.random.rand()
        record = aug.sample(h, w)
        assert record.dtype == np.int32 and record.shape == (len(ia.GRID_MASK_COLUMNS),)
        rec = dict(zip(ia.GRID_MASK_COLUMNS, record.tolist()))
        assert [rec[k] for k in ("d", "length", "st_h", "st_w", "r")] == c["ints"].tolist(), "case %d integers" % i
        assert (rec["active"], rec["mode"], rec["use_h"], rec["use_w"]) == \
            (1, c["cfg"]["mode"], int(c["cfg"]["use_h"]), int(c["cfg"]["use_w"]))
        assert (rec["hh"], rec["ww"], rec["oy"], rec["ox"]) == (int(1.5 * h), int(1.5 * w), (int(1.5 * h) - h) // 2, (int(1.5 * w) - w) // 2)
        assert (rec["rotates"], [rec["a%d" % k] for k in range(6)]) == ia.rotation_terms(rec["r"], rec["ww"], rec["hh"])
        assert np.array_equal(ia.torch_grid_mask(record, h, w).numpy(), c["mask"]), "case %d mask" % i


def test_shipped_parameters_consume_one_draw_and_leave_the_frames(golden):
    frames = [f.copy() for f in golden["frames_a"].astype(np.float32)]
    aug = TRANSFORMS.build(SHIPPED)
    np.random.seed(5)
    out = aug.transform(dict(img=frames))
    after = np.random.uniform()
    np.random.seed(5)
    np.random.rand()
    assert after == np.random.uniform()
    assert all(a is b for a, b in zip(out["img"], frames))


def _pil_mask(h, w, d, length, st_h, st_w, r, use_h, use_w, mode):
    """The reference's steps 3 to 5 with PIL itself."""
    from PIL import Image
    hh, ww = int(1.5 * h), int(1.5 * w)
    mask = np.ones((hh, ww), np.float32)
    if use_h:
        for i in range(hh // d):
            s = d * i + st_h
            mask[s:min(s + length, hh), :] *= 0
    if use_w:
        for i in range(ww // d):
            s = d * i + st_w
            mask[:, s:min(s + length, ww)] *= 0
    mask = np.asarray(Image.fromarray(np.uint8(mask)).rotate(r))
    mask = mask[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w]
    return 1 - mask if mode == 1 else mask


@pytest.mark.parametrize("h,w", [(16, 40), (20, 20), (17, 33)], ids=["16x40", "20x20", "17x33"])
def test_torch_grid_mask_equals_pil_at_every_angle(h, w):
    pytest.importorskip("PIL")
    draws = [(5, 2, 3, 1, True, True, 0), (13, 7, 2, 12, True, False, 0), (2, 1, 1, 0, False, True, 1),
             (min(h, w) - 1, min(h, w) - 2, 0, 4, True, True, 1)]
    bad = []
    for d, length, st_h, st_w, use_h, use_w, mode in draws:
        for r in range(360):
            record = ia.grid_mask_params(h, w, d, length, st_h, st_w, r, use_h, use_w, mode)
            got = ia.torch_grid_mask(record, h, w)
            assert got.dtype == torch.uint8 and got.shape == (h, w)
            if not np.array_equal(got.numpy(), _pil_mask(h, w, d, length, st_h, st_w, r, use_h, use_w, mode)):
                bad.append((d, length, st_h, st_w, r))
    assert not bad, bad


def test_inactive_record_is_all_ones():
    assert ia.torch_grid_mask(np.zeros(len(ia.GRID_MASK_COLUMNS), np.int32), 5, 7).eq(1).all()


def _image_sample(g, frames=None):
    data = dict(ori_shape=(60, 100), cam2img=g["cam2img"], cam2lidar=g["cam2lidar"])
    if frames is not None:
        data["img"] = frames
    return data


IMAGE_AUG = dict(type="ImageAug3D", final_dim=(16, 40), resize_lim=[0.38, 0.55], bot_pct_lim=[0.0, 0.0], rot_lim=[-5.4, 5.4],
                 rand_flip=True, is_train=True)
MASKS = [dict(use_h=True, use_w=True, max_epoch=6, rotate=360, mode=0), dict(use_h=True, use_w=False, max_epoch=6, mode=1),
         dict(use_h=False, use_w=True, max_epoch=6, rotate=360, ratio=1, mode=1), dict(SHIPPED, type=None)]


@pytest.mark.parametrize("form", [(None, False), (torch.bfloat16, True)], ids=["f32", "bf16-cl"])
def test_deferred_equals_eager_through_the_preprocessor(form):
    """ImageAug3D(defer=True) -> GridMask(defer=True) -> process_frames on CPU tensors (the torch path) gives the bits of
    ImageAug3D -> GridMask -> process_imgs under the same seed; a batch of four samples, the last one with the shipped
    prob=0.0, whose plan carries no record."""
    with np.load(os.path.join(os.path.dirname(GOLDEN), "image_aug.npz")) as z:
        g = {k: z[k] for k in ("frames", "cam2img", "cam2lidar")}
    pre = Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=32, pad_value=-1.5, bgr_to_rgb=True, out_dtype=form[0],
                                channels_last=form[1])
    eager_imgs, raw, plans = [], [], []
    for seed, cfg in enumerate(MASKS):
        cfg = {k: v for k, v in cfg.items() if k != "type"}
        runs = []
        for defer in (False, True):
            np.random.seed(40 + seed)
            data = _image_sample(g, list(g["frames"]))
            for step in (dict(IMAGE_AUG, defer=defer), dict(type="GridMask", defer=defer, **cfg)):
                data = TRANSFORMS.build(step).transform(data)
            runs.append((data, np.random.uniform()))
        (e, e_next), (d, d_next) = runs
        assert e_next == d_next
        assert np.array_equal(np.stack(d["img"]), g["frames"])  # pixels left alone
        record = d["img_aug_plan"].grid_mask
        assert (record is None) == (cfg["prob"] == 0.0 if "prob" in cfg else False)
        eager_imgs.append(torch.from_numpy(np.stack(e["img"])).permute(0, 3, 1, 2).contiguous())
        raw.append(torch.from_numpy(np.stack(d["img"])))
        plans.append(d["img_aug_plan"])
    assert any((x == 0).all(1).any() and not (x == 0).all() for x in eager_imgs[:3])  # masks were applied
    want = pre({"inputs": {"img": eager_imgs}})["inputs"]["imgs"]
    before = dict(ia.PATHS)
    got = pre({"inputs": {"img": raw, "img_aug_plan": plans}})["inputs"]["imgs"]
    assert {k: ia.PATHS[k] - before[k] for k in before} == dict(kernel=0, torch=1)
    assert got.shape == (4, 3, 3, 32, 64) and got.dtype == want.dtype and got.stride() == want.stride()
    assert torch.equal(got, want)


def test_record_survives_pickle_and_deepcopy_and_old_pickles_load():
    plan = ia.make_plan([(0.5, (50, 30), (3, 4, 43, 20), True, 5.4), (0.5, (50, 30), (0, 0, 40, 16), False, 0)], (16, 40))
    assert plan.grid_mask is None and pickle.loads(pickle.dumps(plan)).grid_mask is None
    fn, args, state = plan.__reduce__()
    old = fn(*args)
    old.__setstate__(state[:3])  # the three-element state of a pickle made before the record existed
    assert old.grid_mask is None and old.final_dim == (16, 40) and np.array_equal(old, plan)
    record = ia.grid_mask_params(16, 40, 7, 3, 2, 5, 77, True, True, 1)
    plan.grid_mask = record
    results = dict(img_aug_plan=plan, img=[np.zeros((4, 4, 3), np.uint8)])
    for back in (pickle.loads(pickle.dumps(results)), copy.deepcopy(results)):
        p = back["img_aug_plan"]
        assert isinstance(p, ia.AugPlan) and p.final_dim == (16, 40) and np.array_equal(p, plan)
        assert p.grid_mask.dtype == np.int32 and np.array_equal(p.grid_mask, record)
    assert np.array_equal(ia.mask_records([plan, old]), np.stack([record, np.zeros_like(record)]))
    assert ia.mask_records([old, old]) is None


def test_error_paths():
    with pytest.raises(NotImplementedError, match="square"):
        TRANSFORMS.build(dict(type="GridMask", use_h=True, use_w=True, max_epoch=6, offset=True))
    frames = [np.ones((16, 40, 3), np.float32)]
    with pytest.raises(ValueError, match="defer=False"):
        TRANSFORMS.build(dict(SHIPPED, defer=True)).transform(dict(img=frames))
    plan = ia.make_plan([(0.5, (50, 30), (0, 0, 40, 16), False, 0)], (16, 40))
    with pytest.raises(ValueError, match="defer=True"):
        TRANSFORMS.build(dict(SHIPPED, defer=False)).transform(dict(img=frames, img_aug_plan=plan))


def test_record_layout_matches_the_header(tmp_path):
    """The int32[20] record is handed to the entry point as a bfhip_grid_mask: the columns are the struct's ints in order."""
    import subprocess
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    members = {"oy": "crop[0]", "ox": "crop[1]", **{"a%d" % k: "a[%d]" % k for k in range(6)}}
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bevfusion_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(bfhip_grid_mask));\n' +
                   "".join('  printf(" %%zu", offsetof(bfhip_grid_mask, %s));\n' % members.get(c, c) for c in ia.GRID_MASK_COLUMNS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [4 * len(ia.GRID_MASK_COLUMNS)] + [4 * k for k in range(len(ia.GRID_MASK_COLUMNS))]


def test_entry_point_validates_the_record_before_any_launch():
    """Host-only: a malformed record is refused by the host check (no device is touched: the pointers are never followed)."""
    from bevfusion_amd import _lib
    frames = [torch.zeros(1, 37, 61, 3, dtype=torch.uint8)]
    plan = ia.make_plan([(0.38, (23, 14), (0, 0, 27, 13), False, 0)], (13, 27))
    cams, tables = ia.descriptors(frames, [plan], 13, 27)
    scratch = np.zeros(8, np.uint8)
    for column, value, message in (("length", 5, "length=5"), ("st_h", 5, "st_h=5"), ("ox", 14, "outside the canvas")):  # 14 + 27 > ww = 40
        record = ia.grid_mask_params(13, 27, 5, 2, 3, 1, 40)[None].copy()
        record[0, ia.GRID_MASK_COLUMNS.index(column)] = value
        with pytest.raises(RuntimeError, match=message):
            _lib.call("bfhip_image_aug_masked", cams, record.ctypes.data, 1, 1, tables.ctypes.data, tables.ctypes.data,
                      int(tables.size), 13, 27, scratch.ctypes.data, 0, 0, None, None, 0.0, 13, 27, 0, 0, scratch.ctypes.data, None)


# the camera + LiDAR config's train_pipeline from ImageAug3D to PointShuffle, as the reference's config file has it
POINT_CLOUD_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
TRAIN_PIPELINE = [
    dict(type="ImageAug3D", final_dim=[256, 704], resize_lim=[0.38, 0.55], bot_pct_lim=[0.0, 0.0], rot_lim=[-5.4, 5.4],
         rand_flip=True, is_train=True),
    dict(type="BEVFusionGlobalRotScaleTrans", scale_ratio_range=[0.9, 1.1], rot_range=[-0.78539816, 0.78539816],
         translation_std=0.5),
    dict(type="BEVFusionRandomFlip3D"),
    dict(type="PointsRangeFilter", point_cloud_range=POINT_CLOUD_RANGE),
    dict(type="ObjectRangeFilter", point_cloud_range=POINT_CLOUD_RANGE),
    dict(type="ObjectNameFilter", classes=["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle",
                                           "bicycle", "pedestrian", "traffic_cone"]),
    SHIPPED,
    dict(type="PointShuffle"),
]
DEFERRABLE = ("ImageAug3D", "BEVFusionGlobalRotScaleTrans", "BEVFusionRandomFlip3D", "PointsRangeFilter", "GridMask", "PointShuffle")


def _run_pipeline(steps, defer, frames, rig, seed):
    """-> (data, the generator states (numpy, torch) PointShuffle saw)."""
    g = points_aug_cases.golden()
    data = dict(img=list(frames), ori_shape=(900, 1600), cam2img=rig["camera_intrinsics"][0][:2], cam2lidar=rig["camera2lidar"][0][:2],
                points=torch.from_numpy(g["points"].copy()), gt_bboxes_3d=torch.from_numpy(g["boxes"].copy()),
                gt_labels_3d=g["labels"].copy())
    np.random.seed(seed)
    torch.manual_seed(seed)
    seen = None
    for step in steps:
        t = TRANSFORMS.build(dict(step, defer=True) if defer and step["type"] in DEFERRABLE else step)
        if step["type"] == "PointShuffle":
            state = np.random.get_state()
            seen = (state[1].copy(), state[2], torch.get_rng_state().clone())
        data = t.transform(data)
    return data, seen


@pytest.mark.parametrize("prob", [0.0, 1.0])
def test_camera_lidar_train_pipeline_builds_by_name_and_runs_deferred(prob):
    rig = synthetic.camera_rig(batch=1, seed=1, train_aug=False)
    frames = np.ascontiguousarray(synthetic.camera_images_u8(1, 2, 900, 1600, seed=2000)[0].transpose(0, 2, 3, 1))
    steps = [dict(s, prob=prob) if s["type"] == "GridMask" else s for s in TRAIN_PIPELINE]
    assert steps[6] == SHIPPED or prob == 1.0
    eager, seen_e = _run_pipeline(steps, False, [f.astype(np.float32) for f in frames], rig, 12)
    deferred, seen_d = _run_pipeline(steps, True, frames, rig, 12)
    assert np.array_equal(seen_e[0], seen_d[0]) and seen_e[1] == seen_d[1] and torch.equal(seen_e[2], seen_d[2])
    plan = deferred["img_aug_plan"]
    assert (plan.grid_mask is not None) == (prob == 1.0) and plan.final_dim == (256, 704)
    assert "points_aug_plan" in deferred and np.array_equal(np.stack(deferred["img"]), frames)
    assert np.array_equal(np.stack(eager["img_aug_matrix"]), np.stack(deferred["img_aug_matrix"]))
    pre = Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=32, bgr_to_rgb=True)
    want = pre({"inputs": {"img": [torch.from_numpy(np.stack(eager["img"])).permute(0, 3, 1, 2).contiguous()]}})["inputs"]["imgs"]
    got = pre({"inputs": {"img": [torch.from_numpy(frames)], "img_aug_plan": [plan]}})["inputs"]["imgs"]
    assert got.shape == (1, 2, 3, 256, 704) and torch.equal(got, want)
    if prob == 1.0:
        masked = (np.stack(eager["img"]) == 0).all(3)
        assert masked.any() and not masked.all()
