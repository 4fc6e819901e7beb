"""CPU: bevfusion_amd.image_aug -- the host side of ImageAug3D and its plain-torch pixel path.

Everything is compared exactly (np.array_equal / torch.equal): the path is integer arithmetic, the matrix is the reference's own
float32 operations in its order.  The yardsticks are tests/golden/image_aug.npz (the reference's ImageAug3D itself, recorded by
tests/golden/make_image_aug_golden.py) and, where it is installed, PIL."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import image_aug as ia
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor
from bevfusion_amd.registry import MODELS, TRANSFORMS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_aug.npz")
TRAIN = dict(resize_lim=[0.38, 0.55], bot_pct_lim=[0.0, 0.0], rot_lim=[-5.4, 5.4], rand_flip=True, is_train=True)
TEST = dict(resize_lim=[0.38, 0.55], bot_pct_lim=[0.0, 0.0], rot_lim=[0.0, 0.0], rand_flip=False, is_train=False)
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def draws(g):
    for d in range(int(g["n_draws"])):
        yield d, {k: g["draw%d_%s" % (d, k)] for k in ("seed", "train", "resize", "dims", "crop", "flip", "rotate", "matrix", "img",
                                                      "next_uniform")}


def build(g, train, defer=False):
    return TRANSFORMS.build(dict(type="ImageAug3D", final_dim=tuple(int(v) for v in g["final_dim"]), defer=defer,
                                 **(TRAIN if train else TEST)))


def sample(g, frames=None):
    data = dict(ori_shape=tuple(int(v) for v in g["ori_shape"]), cam2img=g["cam2img"], cam2lidar=g["cam2lidar"])
    if frames is not None:
        data["img"] = frames
    return data


def test_registered_as_a_transform_and_not_as_a_model():
    assert TRANSFORMS.get("ImageAug3D") is ia.ImageAug3D and "ImageAug3D" not in MODELS


def test_golden_holds_a_crop_wider_than_the_resized_image(golden):
    """newW < fW in at least one draw: the zero fill at the right edge is part of the recorded pixels."""
    assert any(x["dims"][c][0] < int(golden["final_dim"][1]) for _, x in draws(golden) for c in range(3))


def test_sample_augmentation_reproduces_the_reference_draw_for_draw(golden):
    for d, x in draws(golden):
        aug = build(golden, bool(x["train"]))
        np.random.seed(int(x["seed"]))
        got = [aug.sample_augmentation(sample(golden), c) for c in range(3)]
        nxt = np.random.uniform()
        assert nxt == float(x["next_uniform"]), "draw %d leaves the generator in another state" % d
        for c, (resize, dims, crop, flip, rotate) in enumerate(got):
            assert float(resize) == x["resize"][c] and float(rotate) == x["rotate"][c]
            assert tuple(dims) == tuple(x["dims"][c]) and tuple(crop) == tuple(x["crop"][c]) and bool(flip) == bool(x["flip"][c])


def test_transform_equals_the_reference_pixels_and_matrices(golden):
    frames = [f.astype(np.float32) for f in golden["frames"]]  # float32 holding integers, as the loader delivers
    for d, x in draws(golden):
        aug = build(golden, bool(x["train"]))
        np.random.seed(int(x["seed"]))
        out = aug.transform(sample(golden, list(frames)))
        assert np.random.uniform() == float(x["next_uniform"])
        assert len(out["img"]) == 3 and all(a.dtype == np.float32 and a.shape == (16, 40, 3) for a in out["img"])
        assert np.array_equal(np.stack(out["img"]), x["img"].astype(np.float32)), "draw %d pixels" % d
        got = np.stack(out["img_aug_matrix"])
        assert got.dtype == np.float32 and np.array_equal(got, x["matrix"]), "draw %d matrix" % d


def test_torch_path_on_the_recorded_parameters(golden):
    """Without the sampler: plan from the recorded parameters, uint8 frames, [N, 3, fH, fW] out."""
    for d, x in draws(golden):
        params = [(x["resize"][c], x["dims"][c], x["crop"][c], x["flip"][c], x["rotate"][c]) for c in range(3)]
        plan = ia.make_plan(params, (16, 40))
        assert plan.dtype == np.int32 and plan.shape == (3, 12) and plan.final_dim == (16, 40)
        got = ia.torch_image_aug(torch.from_numpy(golden["frames"]), plan)
        assert got.dtype == torch.uint8 and got.shape == (3, 3, 16, 40)
        assert np.array_equal(got.permute(0, 2, 3, 1).numpy(), x["img"])


def test_plan_survives_slicing_and_pickling():
    plan = ia.make_plan([(0.5, (50, 30), (3, 4, 43, 20), True, 5.4), (0.5, (50, 30), (0, 0, 40, 16), False, 0)], (16, 40))
    assert plan[1:].final_dim == (16, 40) and np.copy(plan[:1]).shape == (1, 12)
    back = pickle.loads(pickle.dumps(plan))
    assert isinstance(back, ia.AugPlan) and back.final_dim == (16, 40) and np.array_equal(back, plan)
    assert plan[0, 5] == 1 and plan[1, 5] == 0 and list(plan[1, 6:]) == [65536, 0, 0, 0, 65536, 0]
    assert not hasattr(plan, "to")  # cast_data leaves it on the host


def _pil_chain(frame, dims, crop, flip, rotate):
    from PIL import Image
    img = Image.fromarray(frame, mode="RGB").resize(dims).crop(crop)
    if flip:
        img = img.transpose(method=Image.FLIP_LEFT_RIGHT)
    return np.array(img.rotate(rotate))


def _pil_cases():
    rs = np.random.RandomState(5)
    cases = []
    for (H, W), (fH, fW) in (((37, 61), (13, 27)), ((90, 160), (24, 64))):
        frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        for resize in (0.38, 0.48, 0.55, 1.0, 1.3):
            newW, newH = int(W * resize), int(H * resize)
            corners = [(max(0, newW - fW) // 2, max(0, newH - fH) // 2), (-3, 2), (newW - fW + 4, 1), (2, -5), (1, newH - fH + 3)]
            for k, rotate in enumerate((0, 5.4, -5.4, 0.3, -0.003, 90, 180)):
                for flip in (False, True):
                    # every crop position with the unrotated image, one (cycling) with every rotation
                    for cx, cy in (corners if rotate == 0 else [corners[k % len(corners)]]):
                        cases.append((frame, (fH, fW), (newW, newH), (cx, cy, cx + fW, cy + fH), flip, rotate))
    frame = rs.randint(0, 256, (37, 61, 3)).astype(np.uint8)  # newH < fH: the crop is taller than the resized image
    cases.append((frame, (20, 27), (30, 18), (1, -1, 28, 19), True, 0.3))
    big = rs.randint(0, 256, (900, 1600, 3)).astype(np.uint8)
    cases.append((big, (256, 704), (int(1600 * 0.4417), int(900 * 0.4417)), (1, 100, 705, 356), True, 5.4))
    return cases


def test_sweep_against_pil_has_no_mismatch():
    pytest.importorskip("PIL")
    bad = []
    for frame, final, dims, crop, flip, rotate in _pil_cases():
        want = _pil_chain(frame, dims, crop, flip, rotate)
        plan = ia.make_plan([(None, dims, crop, flip, rotate)], final)
        got = ia.torch_image_aug(torch.from_numpy(frame)[None], plan)[0].permute(1, 2, 0).numpy()
        if not np.array_equal(got, want):
            bad.append((frame.shape, dims, crop, flip, rotate, int((got != want).sum())))
    assert not bad, bad


def test_coefficients_are_cached_and_windowed():
    full = ia.coefficients(160, 60)
    part = ia.coefficients(160, 60, 7, 20)
    assert ia.coefficients(160, 60, 7, 20) is part
    assert np.array_equal(part[0], full[0][7:27]) and np.array_equal(part[1], full[1][7:27])
    assert np.array_equal(part[2], full[2][7:27, :part[2].shape[1]])
    assert (full[2].sum(1) - (1 << 22)).__abs__().max() <= full[2].shape[1]  # weights sum to one up to the rounding of each


@pytest.mark.parametrize("form", [(None, False), (torch.bfloat16, True)], ids=["f32", "bf16-cl"])
def test_deferred_equals_eager_through_the_preprocessor(golden, form):
    pre = Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=32, pad_value=-1.5, bgr_to_rgb=True, out_dtype=form[0],
                                channels_last=form[1])
    frames = golden["frames"]
    eager_imgs, raw, plans, metas = [], [], [], []
    for seed in (4, 9):  # a batch of two samples, each with its own draw
        np.random.seed(seed)
        e = build(golden, True).transform(sample(golden, list(frames)))
        np.random.seed(seed)
        d = build(golden, True, defer=True).transform(sample(golden, list(frames)))
        assert np.array_equal(np.stack(e["img_aug_matrix"]), np.stack(d["img_aug_matrix"]))
        assert d["img"][0] is frames[0] or np.array_equal(np.stack(d["img"]), frames)  # pixels left alone
        eager_imgs.append(torch.from_numpy(np.stack(e["img"])).permute(0, 3, 1, 2).contiguous())
        raw.append(torch.from_numpy(np.stack(d["img"])))
        plans.append(d["img_aug_plan"])
        metas.append(types.SimpleNamespace(metainfo={}))
    want = pre({"inputs": {"img": eager_imgs}})["inputs"]["imgs"]
    before = dict(ia.PATHS)
    got = pre({"inputs": {"img": raw, "img_aug_plan": plans}, "data_samples": metas})["inputs"]["imgs"]
    assert {k: ia.PATHS[k] - before[k] for k in before} == dict(kernel=0, torch=1)  # a CPU batch takes the torch chain
    assert got.shape == (2, 3, 3, 32, 64) and got.dtype == want.dtype and got.stride() == want.stride()
    assert torch.equal(got, want)
    assert metas[0].metainfo == metas[1].metainfo == dict(batch_input_shape=(32, 64), pad_shape=(32, 64))


def test_supported_query_states_the_kernel_bounds():
    """Host-only: at most 24 taps and source / resized <= 6.25 per axis -- every resize >= 0.2 of the nuScenes frame and of
    small sources; 0.15 is refused and goes to the torch path."""
    from bevfusion_amd import _lib
    lib = _lib.load()
    assert lib.bfhip_image_aug_max_taps() == 24 and lib.bfhip_image_aug_max_cams() >= 24
    for H, W in ((900, 1600), (90, 160), (39, 61)):
        for resize in (0.2, 0.38, 0.48, 0.55, 1.0, 1.3):
            newW, newH = int(W * resize), int(H * resize)
            taps = [ia.coefficients(W, newW)[2].shape[1], ia.coefficients(H, newH)[2].shape[1]]
            assert lib.bfhip_image_aug_supported(H, W, newH, newW, 16, 40, taps[0], taps[1]) == 1, (H, W, resize, taps)
    taps = ia.coefficients(1600, 240)[2].shape[1]
    assert taps > 24 and lib.bfhip_image_aug_supported(900, 1600, 135, 240, 16, 40, taps, taps) == 0


def test_entry_point_validates_the_tables_before_any_launch():
    """Host-only: tables made for a source of 37 rows against a frame of 36 are refused by the host check of every entry (no
    device is touched: the pointers are never followed)."""
    from bevfusion_amd import _lib
    frames = [torch.zeros(1, 36, 61, 3, dtype=torch.uint8)]
    plan = ia.make_plan([(0.38, (23, 14), (0, 0, 27, 13), False, 0)], (13, 27))
    cams, _ = ia.descriptors(frames, [plan], 13, 27)
    tables, _ = ia._pack_tables([(37, 61)], [plan], 13, 27)
    scratch = np.zeros(8, np.uint8)
    with pytest.raises(RuntimeError, match="source 36"):
        _lib.call("bfhip_image_aug", cams, 1, 1, tables.ctypes.data, tables.ctypes.data, int(tables.size), 13, 27,
                  scratch.ctypes.data, 0, 0, None, None, 0.0, 13, 27, 0, 0, scratch.ctypes.data, None)


def test_tables_are_built_with_the_plan_and_travel_with_it(golden):
    """ImageAug3D(defer=True) builds the resampling tables where it makes the plan (a training draw is a new table nearly every
    time: the loader's worker pays for it, not the thread that feeds the GPU).  They survive pickling, are found again by the
    consumer for the same source size, rebuilt for another, and not inherited by a slice."""
    np.random.seed(4)
    plan = build(golden, True, defer=True).transform(sample(golden, list(golden["frames"])))["img_aug_plan"]
    source, buf, refs = plan.tables
    assert source == (60, 100) and buf.dtype == np.int32 and len(refs) == 3
    back = pickle.loads(pickle.dumps(plan))
    assert back.tables[0] == source and np.array_equal(back.tables[1], buf) and back.tables[2] == refs
    assert ia.sample_tables(back, 60, 100) is back.tables
    assert plan[1:].tables is None and np.array(plan).view(ia.AugPlan).tables is None
    packed, flat = ia._pack_tables([(60, 100), (60, 100)], [plan, back], 16, 40)
    assert np.array_equal(packed, np.concatenate([buf, buf])) and flat[3][0] == refs[0][0] + buf.size and flat[3][1:4] == refs[0][1:4]
    other = ia.sample_tables(back, 61, 100)
    assert other[0] == (61, 100) and back.tables is other
    # per camera: the entries of the window are PIL's for that window
    r = refs[0]
    lo, n, k = ia.coefficients(100, int(plan[0, 0]), r[2], r[3])
    block = buf[r[0]:r[0] + r[3] * (2 + r[1])].reshape(r[3], 2 + r[1])
    assert np.array_equal(block[:, 0], lo) and np.array_equal(block[:, 1], n) and np.array_equal(block[:, 2:], k)


def test_coefficient_cache_is_small_and_least_recently_used():
    ia._coeff_cache.clear()
    first = ia.coefficients(1600, 700, 3, 64)
    for out in range(701, 701 + ia._COEFF_CACHE_ENTRIES - 1):
        ia.coefficients(1600, out, 3, 64)
        assert ia.coefficients(1600, 700, 3, 64) is first  # used again: stays
    assert len(ia._coeff_cache) == ia._COEFF_CACHE_ENTRIES
    ia.coefficients(1600, 900, 3, 64)
    assert len(ia._coeff_cache) == ia._COEFF_CACHE_ENTRIES and (1600, 701, 3, 64) not in ia._coeff_cache
    assert (1600, 700, 3, 64) in ia._coeff_cache


def test_environment_switch_is_read_at_import():
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = "import sys; sys.path.insert(0, %r); import bevfusion_amd; from bevfusion_amd import image_aug; print(image_aug.ENABLED)" % root
    for value, want in (("0", "False"), ("1", "True"), (None, "True")):
        env = {k: v for k, v in os.environ.items() if k != "BFHIP_IMG_AUG"}
        if value is not None:
            env["BFHIP_IMG_AUG"] = value
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr[-500:])
