"""CPU: BEVLoadMultiViewImageFromFiles against the recording of the reference's own transform on the demo sample
(tests/golden/make_jpeg_golden.py section (c)), its decoded pixels against Pillow's, the deferred form through ImageAug3D and
Det3DDataPreprocessor, and the host fallback."""
import copy
import hashlib
import json
import os
import warnings

import numpy as np
import pytest
import torch

import jpeg_cases as jc

Z = jc.load()
CAMS = json.loads(str(Z["transform_cams"]))
MATRIX_KEYS = ("cam2img", "lidar2cam", "cam2lidar", "lidar2img", "ori_cam2img")
REF_CASES = json.loads(str(Z["ref_frame_cases"]))


@pytest.fixture(scope="module")
def pkg():
    import bevfusion_amd
    from bevfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        bevfusion_amd.build()
    from bevfusion_amd import data_preprocessor, image_aug, jpeg, loading
    return dict(jpeg=jpeg, loading=loading, image_aug=image_aug, dp=data_preprocessor)


def sample(paths=None, n=None):
    """The demo sample's `images` from the recorded inputs (nested lists of floats, as the .pkl holds them)."""
    cams = CAMS[:n] if n else CAMS
    paths = paths or [jc.FIXTURE] * len(cams)
    return dict(images={c: dict(img_path=p, cam2img=Z["transform_in_cam2img"][i].tolist(),
                                lidar2cam=Z["transform_in_lidar2cam"][i].tolist()) for i, (c, p) in enumerate(zip(cams, paths))})


@pytest.fixture(scope="module")
def loaded(pkg):
    """One defer=False run on the six-camera sample, shared and left unchanged."""
    return pkg["loading"].BEVLoadMultiViewImageFromFiles(to_float32=True, color_type="color").transform(sample())


def test_registered_and_builds_from_the_reference_s_pipeline_dicts(pkg):
    from bevfusion_amd.registry import TRANSFORMS
    assert "BEVLoadMultiViewImageFromFiles" in TRANSFORMS
    for cfg in (dict(type="BEVLoadMultiViewImageFromFiles", to_float32=True, color_type="color", backend_args=None),
                dict(type="BEVLoadMultiViewImageFromFiles", to_float32=True, color_type="color", backend_args=None, num_views=6)):
        t = TRANSFORMS.build(cfg)
        assert (t.to_float32, t.color_type, t.num_ref_frames, t.test_mode, t.set_default_scale, t.defer) == \
            (True, "color", -1, False, True, False)
    assert TRANSFORMS.build(dict(type="BEVLoadMultiViewImageFromFiles")).num_views == 5
    with pytest.raises(NotImplementedError):
        TRANSFORMS.build(dict(type="BEVLoadMultiViewImageFromFiles", color_type="grayscale"))


@pytest.mark.parametrize("key", MATRIX_KEYS)
def test_matrices_equal_the_reference_bit_for_bit(loaded, key):
    want = Z["transform_out_%s" % key]
    got = loaded[key]
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


def test_matrix_dtypes_are_the_reference_s(loaded):
    assert loaded["cam2img"].dtype == np.float32 and loaded["lidar2img"].dtype == np.float32
    assert loaded["cam2lidar"].dtype == np.float64 and loaded["lidar2cam"].dtype == np.float64
    assert loaded["ori_cam2img"] is not loaded["cam2img"]


def test_other_keys(loaded):
    want = json.loads(str(Z["transform_out_shapes"]))
    assert list(loaded["img_shape"]) == want["img_shape"] and list(loaded["ori_shape"]) == want["ori_shape"]
    assert list(loaded["pad_shape"]) == want["pad_shape"]
    assert loaded["scale_factor"] == want["scale_factor"] and loaded["num_views"] == want["num_views"]
    assert loaded["num_ref_frames"] == want["num_ref_frames"]
    assert loaded["img_path"] == loaded["filename"] == [jc.FIXTURE] * len(CAMS)
    assert len(loaded["img"]) == want["n_img"] and str(loaded["img"][0].dtype) == want["img_dtype"]
    assert list(loaded["img"][0].shape) == want["img0_shape"]
    cfg = loaded["img_norm_cfg"]
    assert cfg["to_rgb"] is False and cfg["mean"].dtype == np.float32 and np.array_equal(cfg["mean"], np.zeros(3))
    assert cfg["std"].dtype == np.float32 and np.array_equal(cfg["std"], np.ones(3))


def test_pixels_match_the_recorded_pillow_hash(pkg, loaded):
    img = loaded["img"][0]
    assert img.dtype == np.float32
    assert hashlib.sha256(np.ascontiguousarray(img.astype(np.uint8)).tobytes()).hexdigest() == str(Z["fixture_sha256"])
    assert np.array_equal(img, img.astype(np.uint8))
    raw = pkg["loading"].BEVLoadMultiViewImageFromFiles().transform(sample(n=1))
    assert raw["img"][0].dtype == np.uint8 and np.array_equal(raw["img"][0], img.astype(np.uint8))
    assert "scale_factor" not in pkg["loading"].BEVLoadMultiViewImageFromFiles(set_default_scale=False).transform(sample(n=1))


@pytest.mark.parametrize("case", REF_CASES, ids=["seed%d_frames%d_refs%d_%s" % (c["seed"], c["frames"], c["refs"],
                                                                                "test" if c["test_mode"] else "train")
                                                  for c in REF_CASES])
def test_reference_frame_choice(pkg, case):
    V = 2
    rs = np.random.RandomState(50 + case["frames"])
    d = sample(n=V)
    d["img_filename"] = ["%d_%d" % (f, v) for f in range(case["frames"]) for v in range(V)]
    d["ego2global"] = [np.eye(4) + 0.01 * rs.standard_normal((4, 4)) for _ in range(case["frames"])]
    d["lidar2cam"] = [rs.standard_normal((4, 4)) for _ in range(case["frames"] * V)]
    d["cam2img"] = [rs.standard_normal((3, 3)) for _ in range(case["frames"] * V)]
    ego = np.stack(d["ego2global"])
    np.random.seed(case["seed"])
    out = pkg["loading"].BEVLoadMultiViewImageFromFiles(num_views=V, num_ref_frames=case["refs"],
                                                       test_mode=case["test_mode"]).transform(d)
    assert repr(np.random.uniform()) == case["next_uniform"]
    assert [int(n.split("_")[0]) for n in out["img_filename"][::V]] == case["choices"]
    assert np.array_equal(np.stack(out["ego2global"]), ego[case["choices"]])
    assert out["lidar2cam"].shape == (V, 4, 4) and len(out["img"]) == V  # the files still come from `images`
    assert out["num_ref_frames"] == case["refs"]


def test_frames_of_different_sizes_are_zero_padded(pkg, tmp_path):
    streams = dict((n, b) for n, b, _ in jc.streams())
    pixels = dict((n, p) for n, _, p in jc.streams())
    names = ["420_17x23_q75", "420_33x9_q75"]
    paths = []
    for n in names:
        (tmp_path / (n + ".jpg")).write_bytes(streams[n])
        paths.append(str(tmp_path / (n + ".jpg")))
    out = pkg["loading"].BEVLoadMultiViewImageFromFiles().transform(sample(paths, n=2))
    assert out["img_shape"] == (23, 33) and [i.shape for i in out["img"]] == [(23, 33, 3)] * 2
    for img, n in zip(out["img"], names):
        h, w = pixels[n].shape[:2]
        assert np.array_equal(img[:h, :w], pixels[n]) and not img[h:].any() and not img[:, w:].any()
    deferred = pkg["loading"].BEVLoadMultiViewImageFromFiles(defer=True).transform(sample(paths, n=2))["img"]
    assert deferred.shape == (2, 23, 33, 3) and deferred.padded()
    assert np.array_equal(deferred.decode_host().numpy(), np.stack(out["img"]))


def test_deferred_load_then_deferred_image_aug_builds_its_plan(pkg):
    load = pkg["loading"].BEVLoadMultiViewImageFromFiles(defer=True)
    data = load.transform(sample(n=2))
    frames = data["img"]
    assert isinstance(frames, pkg["jpeg"].JpegFrames) and len(frames) == 2 and frames.shape == (2, 900, 1600, 3)
    assert frames.coef.dtype == np.int16 and frames.coef.size == frames.offsets[-1] == 2 * (frames.headers[0].coef_bytes // 2)
    aug = pkg["image_aug"].ImageAug3D(final_dim=[256, 704], resize_lim=[0.48, 0.48], bot_pct_lim=[0.0, 0.0], rot_lim=[0.0, 0.0],
                                      rand_flip=False, is_train=False, defer=True)
    data = aug.transform(data)
    assert data["img"] is frames and len(data["img_aug_matrix"]) == 2
    plan = data["img_aug_plan"]
    assert plan.final_dim == (256, 704) and len(plan) == 2 and plan.tables[0] == (900, 1600)
    with pytest.raises(ValueError):
        pkg["loading"].BEVLoadMultiViewImageFromFiles(defer=True, to_float32=True)


def small_sample(tmp_path, names):
    streams = dict((n, b) for n, b, _ in jc.streams())
    paths = []
    for i, n in enumerate(names):
        p = tmp_path / ("%d_%s.jpg" % (i, n))
        p.write_bytes(streams[n])
        paths.append(str(p))
    return sample(paths, n=len(names))


def test_preprocessor_takes_jpeg_frames_like_the_decoded_block(pkg, tmp_path):
    """CPU end to end: a batch of JpegFrames gives the batch the decoded blocks give, with and without an ImageAug3D plan."""
    dp, ia = pkg["dp"], pkg["image_aug"]
    names = [["420_17x23_q75", "420_17x23_q30"], ["420_17x23_q100", "420_17x23_q75_restart"]]
    deferred = [pkg["loading"].BEVLoadMultiViewImageFromFiles(defer=True).transform(small_sample(tmp_path, n)) for n in names]
    eager = [pkg["loading"].BEVLoadMultiViewImageFromFiles().transform(small_sample(tmp_path, n)) for n in names]
    blocks = [torch.from_numpy(np.stack(e["img"])) for e in eager]
    mod = dp.Det3DDataPreprocessor(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], pad_size_divisor=8)
    got = mod(dict(inputs=dict(img=[d["img"] for d in deferred])))["inputs"]["imgs"]
    want = mod(dict(inputs=dict(img=[b.permute(0, 3, 1, 2) for b in blocks])))["inputs"]["imgs"]
    assert got.shape == (2, 2, 3, 24, 24) and torch.equal(got, want)
    aug = ia.ImageAug3D(final_dim=[8, 12], resize_lim=[0.6, 0.7], bot_pct_lim=[0.0, 0.0], rot_lim=[-5.4, 5.4], rand_flip=True,
                        is_train=True, defer=True)
    np.random.seed(4)
    plans = [aug.transform(d)["img_aug_plan"] for d in deferred]
    got = mod(dict(inputs=dict(img=[d["img"] for d in deferred], img_aug_plan=plans)))["inputs"]["imgs"]
    want = mod(dict(inputs=dict(img=blocks, img_aug_plan=plans)))["inputs"]["imgs"]
    assert got.shape == (2, 2, 3, 8, 16) and torch.equal(got, want)
    assert isinstance(deferred[0]["img"], pkg["jpeg"].JpegFrames)  # the input is left as it came


def test_unsupported_frame_falls_back_to_the_host_with_one_warning(pkg, tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    monkeypatch.setattr(pkg["loading"], "_warned_fallback", False)
    good = dict((n, b) for n, b, _ in jc.streams())["420_17x23_q75"]
    for name, data in jc.unsupported_streams():
        (tmp_path / (name + ".jpg")).write_bytes(data)
    (tmp_path / "good.jpg").write_bytes(good)
    load = pkg["loading"].BEVLoadMultiViewImageFromFiles(defer=True)
    with pytest.warns(UserWarning, match="not taken by the fused JPEG decoder"):
        out = load.transform(sample([str(tmp_path / "progressive.jpg"), str(tmp_path / "grayscale.jpg")], n=2))
    img = out["img"]
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (2, 20, 24, 3)
    assert np.array_equal(img[0], Z["unsupported_progressive_pixels"]) and np.array_equal(img[1], Z["unsupported_grayscale_pixels"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # issued once
        out = load.transform(sample([str(tmp_path / "good.jpg"), str(tmp_path / "progressive.jpg")], n=2))
    assert out["img"].shape == (2, 23, 24, 3) and out["img_shape"] == (23, 24)
    # such a block goes through the preprocessor as any raw block does
    mod = pkg["dp"].Det3DDataPreprocessor(pad_size_divisor=1)
    got = mod(dict(inputs=dict(img=[img])))
    assert got["inputs"]["imgs"].shape == (1, 2, 3, 20, 24)


def test_jpeg_frames_pickle_and_deep_copy(pkg, tmp_path):
    """What a loader's worker hands back: the deferred frames survive pickling and copy.deepcopy with the same bits."""
    import pickle
    frames = pkg["loading"].BEVLoadMultiViewImageFromFiles(defer=True).transform(
        small_sample(tmp_path, ["420_17x23_q75", "420_17x23_q30"]))["img"]
    want = frames.decode_host()
    for other in (pickle.loads(pickle.dumps(frames)), copy.deepcopy(frames)):
        assert other.shape == frames.shape and torch.equal(other.decode_host(), want)
