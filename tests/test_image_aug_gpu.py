"""GPU: csrc/image_aug.hip (bfhip_image_aug) through Det3DDataPreprocessor and image_aug.fused_image_aug.

The oracle is image_aug.torch_image_aug on the CPU -- held bit for bit to PIL and to the reference's recorded output by
tests/test_image_aug_cpu.py -- followed by the preprocessor's chain restated in torch (test_preprocess_gpu.oracle).  The kernels
are the same integer arithmetic and then the same fp32 operations in the same order, so every comparison is torch.equal."""
import os
import types

import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, synthetic
from bevfusion_amd import data_preprocessor as dp
from bevfusion_amd import image_aug as ia
from test_preprocess_gpu import FORM_IDS, FORMS, MEAN, STD, oracle, reproducible_library  # noqa: F401

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_aug.npz")
# source -> final_dim; the third spans three 64-column tiles and two 16-row tiles of the resize kernel, and at 0.38 both newW < fW
# and newH < fH
SHAPES = {"37x61": ((37, 61), (13, 27)), "90x160": ((90, 160), (24, 64)), "50x230": ((50, 230), (20, 150))}
PADDED = {"37x61": (32, 32), "90x160": (32, 64), "50x230": (32, 160)}
ROTATIONS = {"rotating": (0, 5.4, -5.4, 0.3, 90, 180), "none rotates": (0,) * 6, "one rotates": (0, 0, 0, 0, 5.4, 0)}


def plans_of(shape, rotations):
    """B = 2 samples of N = 3 cameras, a different plan per camera: resize 0.38 (most taps; newW < fW), 1.0 and 1.3, a crop
    over each of the four edges, mirrored and not."""
    (H, W), (fH, fW) = SHAPES[shape]
    cams = []
    for k, (resize, where, flip) in enumerate([(0.38, "centre", False), (1.0, "left", True), (1.3, "right", False),
                                               (0.48, "top", True), (0.55, "bottom", False), (1.3, "centre", True)]):
        newW, newH = int(W * resize), int(H * resize)
        cx, cy = dict(centre=(max(0, newW - fW) // 2, max(0, newH - fH) // 2), left=(-3, 2), right=(newW - fW + 4, 1), top=(2, -5),
                      bottom=(1, newH - fH + 3))[where]
        cams.append((resize, (newW, newH), (cx, cy, cx + fW, cy + fH), flip, rotations[k]))
    assert cams[0][1][0] < fW
    return [ia.make_plan(cams[:3], (fH, fW)), ia.make_plan(cams[3:], (fH, fW))]


def frames_of(shape, B=2, N=3, seed=21):
    H, W = SHAPES[shape][0]
    g = torch.Generator().manual_seed(seed)
    frames = [torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8) for _ in range(B)]
    for f in frames:
        f.view(-1)[0], f.view(-1)[-1] = 0, 255
    return frames


_aug, _want = {}, {}


def augmented(shape, rot):
    """The torch path on the CPU, once per (shape, rotation set): list of uint8 [N, 3, fH, fW]."""
    if (shape, rot) not in _aug:
        _aug[shape, rot] = [ia.torch_image_aug(f, p) for f, p in zip(frames_of(shape), plans_of(shape, ROTATIONS[rot]))]
    return _aug[shape, rot]


def want_of(shape, rot, swap, norm):
    key = (shape, rot, swap, norm)
    if key not in _want:
        _want[key] = oracle(augmented(shape, rot), MEAN if norm else None, STD if norm else None, swap, 32, -1.5)
    return _want[key]


def run(frames, plans, dev, kernel=True, **kw):
    """The module on `dev` with the deferred plans -> imgs on the CPU; asserts which path took the batch."""
    m = dp.Det3DDataPreprocessor(**kw).to(dev)
    before = dict(ia.PATHS)
    out = m({"inputs": {"img": frames, "img_aug_plan": plans}})["inputs"]["imgs"]
    took = {k: ia.PATHS[k] - before[k] for k in before}
    assert took == (dict(kernel=1, torch=0) if kernel else dict(kernel=0, torch=1)), took
    assert out.is_cuda
    if kw.get("channels_last"):
        B, N, C, H, W = out.shape
        flat = out.reshape(B * N, C, H, W)
        assert flat.is_contiguous(memory_format=torch.channels_last) and flat.data_ptr() == out.data_ptr()
    else:
        assert out.is_contiguous()
    return out.cpu()


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("swap", [False, True], ids=["rgb", "swap"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rot", list(ROTATIONS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_small_shapes_every_form(dev, shape, rot, form, swap, norm):
    want = want_of(shape, rot, swap, norm)
    assert want.shape == (2, 3, 3) + PADDED[shape]
    out = run(frames_of(shape), plans_of(shape, ROTATIONS[rot]), dev, mean=MEAN if norm else None, std=STD if norm else None,
              pad_size_divisor=32, pad_value=-1.5, bgr_to_rgb=swap, out_dtype=form[0], channels_last=form[1])
    assert out.dtype == (form[0] or torch.float32)
    assert torch.equal(out, want if form[0] is None else want.to(form[0]))


def test_kernel_equals_the_reference_recording(dev):
    """tests/golden/image_aug.npz: the reference's own pixels (PIL), normalised in torch, for every recorded draw."""
    g = np.load(GOLDEN)
    frames = [torch.from_numpy(g["frames"])]
    for d in range(int(g["n_draws"])):
        x = {k: g["draw%d_%s" % (d, k)] for k in ("resize", "dims", "crop", "flip", "rotate", "img")}
        plan = ia.make_plan([(x["resize"][c], x["dims"][c], x["crop"][c], x["flip"][c], x["rotate"][c]) for c in range(3)], (16, 40))
        want = oracle([torch.from_numpy(x["img"]).permute(0, 3, 1, 2)], MEAN, STD, True, 1, 0)
        out = run(frames, [plan], dev, mean=MEAN, std=STD, bgr_to_rgb=True)
        assert torch.equal(out, want), "draw %d" % d


@pytest.mark.parametrize("margin", [64, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("rot", ["rotating", "none rotates"])
def test_every_element_written_once_nothing_outside(dev, rot, form, margin):
    """Output and intermediate sit in the middle of sentinel-filled buffers.  The output's sentinel is a NaN bit pattern that
    neither the pixels nor pad_value can produce, so the margins keep it and no output element does; the intermediate's
    margins keep theirs, and that all of it was written shows in the output being right although it started as 0xA5."""
    out_dtype, pixel_major = form
    bf16 = out_dtype == torch.bfloat16
    shape = "90x160"
    frames = [f.to(dev) for f in frames_of(shape)]
    plans = plans_of(shape, ROTATIONS[rot])
    want = want_of(shape, rot, False, True)
    n, n_mid = want.numel(), 6 * 3 * 24 * 64
    bits, sentinel = (torch.int16, 0x7fc1) if bf16 else (torch.int32, 0x7fc12345)
    buf = torch.full((margin + n + margin,), sentinel, dtype=bits, device=dev)
    mbuf = torch.full((margin + n_mid + margin,), 0xA5, dtype=torch.uint8, device=dev)
    inner = buf[margin:margin + n]
    assert (inner.data_ptr() % 16 == 0) == (margin == 64)
    out = ia.fused_image_aug(frames, plans, None, (MEAN, STD), False, 32, -1.5, out_dtype, pixel_major,
                             store=inner.view(torch.bfloat16 if bf16 else torch.float32), mid=mbuf[margin:margin + n_mid])
    torch.cuda.synchronize()
    assert (buf[:margin] == sentinel).all() and (buf[margin + n:] == sentinel).all()
    assert (mbuf[:margin] == 0xA5).all() and (mbuf[margin + n_mid:] == 0xA5).all()
    assert not (inner == sentinel).any()
    assert torch.equal(out.cpu(), want.to(torch.bfloat16) if bf16 else want)


@pytest.mark.parametrize("rotating", [False, True], ids=["none rotates", "last rotates"])
def test_more_cameras_than_one_launch_holds(dev, rotating):
    n = _lib.load().bfhip_image_aug_max_cams() + 1
    g = torch.Generator().manual_seed(9)
    frames = [torch.randint(0, 256, (1, 12, 20, 3), generator=g, dtype=torch.uint8) for _ in range(n)]
    plans = [ia.make_plan([(0.5, (10, 6), (k % 3, 0, k % 3 + 9, 5), bool(k & 1), 5.4 if rotating and k == n - 1 else 0)], (5, 9))
             for k in range(n)]
    want = oracle([ia.torch_image_aug(f, p) for f, p in zip(frames, plans)], MEAN, STD, False, 1, 0)
    assert want.shape == (n, 1, 3, 5, 9)
    assert torch.equal(run(frames, plans, dev, mean=MEAN, std=STD), want)


def test_plan_above_the_tap_bound_goes_through_torch(dev):
    """resize 0.15: source / resized = 6.67 per axis and up to 28 taps, above what the kernel stages -> the query says no, the
    torch chain serves the batch on the device and the bits are the same."""
    lib = _lib.load()
    assert lib.bfhip_image_aug_max_taps() == 24
    (H, W), final = SHAPES["90x160"]
    assert lib.bfhip_image_aug_supported(H, W, int(H * 0.2), int(W * 0.2), final[0], final[1], 21, 21) == 1  # resize 0.2
    assert lib.bfhip_image_aug_supported(900, 1600, 180, 320, 256, 704, 21, 21) == 1
    assert lib.bfhip_image_aug_supported(H, W, 13, 24, final[0], final[1], 28, 28) == 0
    frames = frames_of("90x160", B=1)
    plan = ia.make_plan([(0.15, (24, 13), (-20, -5, 44, 19), k == 1, 0.3 * k) for k in range(3)], final)
    want = oracle([ia.torch_image_aug(frames[0], plan)], MEAN, STD, False, 32, 0)
    assert torch.equal(run(frames, [plan], dev, kernel=False, mean=MEAN, std=STD, pad_size_divisor=32), want)


def test_switch_off_and_unsupported_inputs_give_the_same_bits(dev, monkeypatch):
    shape, rot = "37x61", "rotating"
    frames, plans = frames_of(shape), plans_of(shape, ROTATIONS[rot])
    kw = dict(mean=MEAN, std=STD, pad_size_divisor=32, pad_value=-1.5)
    want = want_of(shape, rot, False, True)
    monkeypatch.setattr(ia, "ENABLED", False)
    for form in FORMS:
        out = run(frames, plans, dev, kernel=False, out_dtype=form[0], channels_last=form[1], **kw)
        assert torch.equal(out, want if form[0] is None else want.to(form[0]))
    monkeypatch.setattr(ia, "ENABLED", True)
    assert torch.equal(run(frames, plans, dev, kernel=True, **kw), want)
    # what the kernel does not take goes the same way with the switch on: frames that are a strided view, float32 frames
    strided = [f.to(dev).transpose(1, 2).contiguous().transpose(1, 2) for f in frames]
    assert not strided[0].is_contiguous()
    assert torch.equal(run(strided, plans, dev, kernel=False, **kw), want)
    assert torch.equal(run([f.float() for f in frames], plans, dev, kernel=False, **kw), want)
    # one [B, N, H, W, 3] tensor instead of the list, and a batch without a plan is untouched by all this
    assert torch.equal(run(torch.stack(frames), plans, dev, kernel=True, **kw), want)
    before = dict(ia.PATHS)
    dp.Det3DDataPreprocessor(**kw).to(dev)({"inputs": {"img": augmented(shape, rot)}})
    assert ia.PATHS == before


def test_entry_point_rejects_a_table_that_reads_outside_the_source(dev, monkeypatch):
    frames = [f.to(dev) for f in frames_of("37x61", B=1)]
    plan = plans_of("37x61", ROTATIONS["none rotates"])[:1]
    taller = [torch.zeros(3, 36, 61, 3, dtype=torch.uint8, device=dev)]  # tables made for 37 rows, a source of 36
    real = ia._pack_tables
    with monkeypatch.context() as mp:
        mp.setattr(ia, "_pack_tables", lambda shapes, plans, fH, fW: real([(37, 61)], plans, fH, fW))
        with pytest.raises(RuntimeError, match="source 36"):
            ia.fused_image_aug(taller, plan)
    assert ia.fused_image_aug(frames, plan).shape == (1, 3, 3, 13, 27)


def test_test_step_on_raw_frames_equals_test_step_on_augmented_frames(dev, reproducible_library):
    """Camera + LiDAR model at batch 1: six raw 900 x 1600 frames with the deferred test-time plan give the boxes, scores and
    labels of the frames the torch path augmented on the host."""
    from bevfusion_amd.bevfusion import nuscenes_config
    from bevfusion_amd.registry import MODELS, TRANSFORMS
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config()).to(dev).eval()
    raw = np.ascontiguousarray(synthetic.camera_images_u8(1, 6, 900, 1600, seed=2000)[0].transpose(0, 2, 3, 1))
    points = [torch.from_numpy(synthetic.lidar_sweep(40000, seed=1000))]
    rig = synthetic.camera_rig(batch=1, seed=1, train_aug=False)
    cfg = dict(type="ImageAug3D", final_dim=(256, 704), resize_lim=[0.48, 0.48], bot_pct_lim=[0.0, 0.0], rot_lim=[0.0, 0.0],
               rand_flip=False, is_train=False)
    data = dict(img=list(raw), ori_shape=(900, 1600), cam2img=rig["camera_intrinsics"][0], cam2lidar=rig["camera2lidar"][0])
    deferred = TRANSFORMS.build(dict(cfg, defer=True)).transform(dict(data))
    plan = deferred["img_aug_plan"]
    assert plan.shape == (6, 12) and not plan[:, 5].any() and tuple(plan[0, :2]) == (768, 432)
    eager = ia.torch_image_aug(torch.from_numpy(raw), plan)
    meta = {dst: rig[src][0] for src, dst in (("lidar2image", "lidar2img"), ("camera_intrinsics", "cam2img"),
                                               ("camera2lidar", "cam2lidar"), ("lidar_aug_matrix", "lidar_aug_matrix"))}
    meta["img_aug_matrix"] = np.stack(deferred["img_aug_matrix"])
    samples = [types.SimpleNamespace(metainfo=dict(meta))]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = model.test_step({"inputs": {"img": [eager], "points": points}, "data_samples": samples})
        before = dict(ia.PATHS)
        out = model.test_step({"inputs": {"img": [torch.from_numpy(raw)], "img_aug_plan": [plan], "points": points},
                               "data_samples": samples})
    assert ia.PATHS["kernel"] == before["kernel"] + 1 and ia.PATHS["torch"] == before["torch"]
    assert samples[0].metainfo["batch_input_shape"] == (256, 704) and samples[0].metainfo["pad_shape"] == (256, 704)
    assert len(ref) == len(out) == 1 and ref[0]["bboxes_3d"].shape[0] > 0
    for key in ("bboxes_3d", "scores_3d", "labels_3d"):
        assert torch.equal(out[0][key], ref[0][key]), key
