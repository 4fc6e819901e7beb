"""GPU: GridMask in the deferred camera kernels (csrc/image_aug.hip, bfhip_image_aug_masked) through Det3DDataPreprocessor and
image_aug.fused_image_aug.

The yardstick is the torch path on the same device (BFHIP_IMG_AUG=0: image_aug.torch_image_aug with torch_grid_mask, then the
preprocessor's own path), which tests/test_grid_mask_cpu.py holds to the reference's recording and to PIL.  The mask is integer
work and the normalisation is the same fp32 expression on both sides, so every comparison is torch.equal."""
import types

import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, synthetic
from bevfusion_amd import image_aug as ia
from test_image_aug_gpu import run
from test_preprocess_gpu import FORM_IDS, FORMS, MEAN, STD

pytestmark = pytest.mark.gpu
H, W = 60, 100
N_REC = len(ia.GRID_MASK_COLUMNS)


def frames_of(B, N=3, seed=31):
    g = torch.Generator().manual_seed(seed)
    frames = [torch.randint(1, 256, (N, H, W, 3), generator=g, dtype=torch.uint8) for _ in range(B)]
    for f in frames:
        f.view(-1)[0], f.view(-1)[-1] = 0, 255
    return frames


def plans_of(final, B, N=3, rotations=(0, 5.4, 0, -5.4, 90, 0.3)):
    """Camera k of the batch: one of three resizes, a crop that moves with k (every fourth hangs over the right edge), every
    other one mirrored, rotated by rotations[k % len]."""
    fH, fW = final
    plans = []
    for b in range(B):
        cams = []
        for v in range(N):
            k = b * N + v
            resize = (0.45, 0.55, 0.5)[k % 3]
            newW, newH = int(W * resize), int(H * resize)
            cx = newW - fW + 4 if k % 4 == 3 else (3 * k) % (newW - fW + 1)
            cy = (2 * k) % (newH - fH + 1)
            cams.append((resize, (newW, newH), (cx, cy, cx + fW, cy + fH), bool(k & 1), rotations[k % len(rotations)]))
        plans.append(ia.make_plan(cams, final))
    return plans


def with_masks(plans, records):
    """records: per sample None, "inactive" or (d, length, st_h, st_w, r, use_h, use_w, mode)."""
    fH, fW = plans[0].final_dim
    for plan, rec in zip(plans, records):
        if rec == "inactive":
            plan.grid_mask = np.zeros(N_REC, np.int32)
        elif rec is not None:
            plan.grid_mask = ia.grid_mask_params(fH, fW, *rec)
    return plans


def kernel_and_torch(frames, plans, dev, monkeypatch, **kw):
    """The batch through the kernels and through the torch chain on the same device; asserts the bits agree -> the result."""
    got = run(frames, plans, dev, kernel=True, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(ia, "ENABLED", False)
        want = run(frames, plans, dev, kernel=False, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want)
    return got


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("final,divisor", [((16, 40), 32), ((16, 37), 1)], ids=["16x40-pad32", "16x37"])
def test_masked_batch_every_form(dev, monkeypatch, final, divisor, form):
    """(16, 40) padded to 32 x 64: the pad rows and columns hold pad_value also where the mask is 0; (16, 37) unpadded: a partial
    last run of 5 pixels and element-wise stores."""
    fH, fW = final
    plans = with_masks(plans_of(final, 2), [(5, 2, 3, 1, 0, True, True, 0), (7, 4, 6, 0, 33, True, True, 1)])
    out = kernel_and_torch(frames_of(2), plans, dev, monkeypatch, mean=MEAN, std=STD, pad_size_divisor=divisor, pad_value=-1.5,
                           out_dtype=form[0], channels_last=form[1])
    Hp, Wp = -(-fH // divisor) * divisor, -(-fW // divisor) * divisor
    assert out.shape == (2, 3, 3, Hp, Wp)
    pad = torch.ones(Hp, Wp, dtype=torch.bool)
    pad[:fH, :fW] = False
    assert (out[..., pad].float() == -1.5).all()
    zero = ((0.0 - torch.tensor(MEAN)) / torch.tensor(STD)).to(out.dtype)  # what a masked pixel becomes
    for b, plan in enumerate(plans):
        masked = ia.torch_grid_mask(plan.grid_mask, fH, fW) == 0
        assert masked.any() and not masked.all()
        for c in range(3):
            assert (out[b, :, c, :fH, :fW][:, masked] == zero[c]).all()


@pytest.mark.parametrize("swap,norm", [(False, True), (True, False)], ids=["rgb-norm", "swap-raw"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_mixed_batch(dev, monkeypatch, form, swap, norm):
    """B = 4, N = 3: a sample without a record, one with an inactive record, mode 0 unrotated and mode 1 at 77 degrees; among
    each sample's cameras one that rotates, one that is mirrored and one that is neither."""
    plans = with_masks(plans_of((16, 40), 4, rotations=(5.4, 0, 0)),
                       [None, "inactive", (6, 3, 2, 5, 0, True, False, 0), (9, 5, 8, 3, 77, True, True, 1)])
    flips, rots = np.stack(plans)[:, :, 4], np.stack(plans)[:, :, 5]
    assert all(((f == 1) & (r == 0)).any() and ((f == 0) & (r == 0)).any() and (r == 1).any() for f, r in zip(flips, rots))
    kernel_and_torch(frames_of(4), plans, dev, monkeypatch, mean=MEAN if norm else None, std=STD if norm else None,
                     pad_size_divisor=32, pad_value=-1.5, bgr_to_rgb=swap, out_dtype=form[0], channels_last=form[1])


@pytest.mark.parametrize("r", [0, 200], ids=["mask unrotated", "mask rotated"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_no_frame_rotates_but_a_mask_is_active(dev, monkeypatch, form, r):
    """Without a mask this batch takes the preprocessing kernel as its second launch; with one it takes the finish kernel."""
    plans = with_masks(plans_of((16, 40), 2, rotations=(0,)), [(4, 2, 1, 3, r, True, True, 0), None])
    assert not np.stack(plans)[:, :, 5].any()
    kernel_and_torch(frames_of(2), plans, dev, monkeypatch, mean=MEAN, std=STD, pad_size_divisor=32, out_dtype=form[0],
                     channels_last=form[1])


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_launch_boundary_inside_a_sample(dev, monkeypatch, form):
    """B = 11, N = 3: 33 cameras, so the second launch chunk begins with the last camera of sample 10; every sample its own
    record."""
    assert _lib.load().bfhip_image_aug_max_cams() == 32
    records = [(2 + b, 1 + b // 2, b % (2 + b), (3 * b) % (2 + b), (0, 77, 180, 291)[b % 4], b % 3 != 1, b % 3 != 2, b & 1)
               for b in range(11)]
    plans = with_masks(plans_of((16, 40), 11), records)
    kernel_and_torch(frames_of(11), plans, dev, monkeypatch, mean=MEAN, std=STD, out_dtype=form[0], channels_last=form[1])


@pytest.mark.parametrize("margin", [64, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_element_written_once_nothing_outside(dev, monkeypatch, form, margin):
    """As tests/test_image_aug_gpu.py with a mask on: output and intermediate sit in the middle of sentinel-filled buffers; the
    output's sentinel is a NaN bit pattern neither the pixels nor pad_value can produce."""
    out_dtype, pixel_major = form
    bf16 = out_dtype == torch.bfloat16
    frames = [f.to(dev) for f in frames_of(2)]
    plans = with_masks(plans_of((16, 40), 2), [(5, 2, 3, 1, 0, True, True, 1), (7, 4, 6, 0, 33, True, True, 0)])
    with monkeypatch.context() as mp:
        mp.setattr(ia, "ENABLED", False)
        want = run(frames, plans, dev, kernel=False, mean=MEAN, std=STD, pad_size_divisor=32, pad_value=-1.5)
    n, n_mid = want.numel(), 6 * 3 * 16 * 40
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


def test_entry_point_rejects_a_malformed_record(dev):
    frames = [f.to(dev) for f in frames_of(1)]
    good = (5, 2, 3, 1, 0, True, True, 0)
    for column, value, message in (("length", 5, "length=5"), ("st_w", 5, "st_w=5"), ("st_h", -1, "st_h=-1"), ("d", 1, "d=1"),
                                   ("oy", 9, "outside the canvas"), ("ww", 49, "outside the canvas")):
        plans = with_masks(plans_of((16, 40), 1), [good])
        plans[0].grid_mask[ia.GRID_MASK_COLUMNS.index(column)] = value
        out = torch.full((3 * 3 * 16 * 40,), 7.0, device=dev)
        with pytest.raises(RuntimeError, match=message):
            ia.fused_image_aug(frames, plans, store=out)
        torch.cuda.synchronize()
        assert (out == 7.0).all()  # nothing was launched
    assert ia.fused_image_aug(frames, with_masks(plans_of((16, 40), 1), [good])).shape == (1, 3, 3, 16, 40)


@pytest.mark.parametrize("rotations", [(0, 5.4, 0), (0,)], ids=["rotating", "none rotates"])
def test_without_an_active_record_the_output_is_that_of_bfhip_image_aug(dev, rotations):
    frames = [f.to(dev) for f in frames_of(2)]
    plans = plans_of((16, 40), 2, rotations=rotations)
    cams, tables = ia.descriptors(frames, plans, 16, 40)
    tables_dev = torch.from_numpy(tables).to(dev)
    mean, std = _lib.host_f32(MEAN), _lib.host_f32(STD)
    mid = torch.empty(6 * 3 * 16 * 40, dtype=torch.uint8, device=dev)
    tail = (2, 3, tables.ctypes.data, tables_dev.data_ptr(), int(tables.size), 16, 40, mid.data_ptr(), 0, 1, mean, std, -1.5, 32, 64,
            1, 1)
    outs = []
    inactive = np.zeros((2, N_REC), np.int32)
    inactive[:, 1:] = 12345  # an inactive record is not read
    for masks in ("plain", None, inactive):
        out = torch.full((6 * 3 * 32 * 64,), float("nan"), dtype=torch.bfloat16, device=dev)
        if isinstance(masks, str):
            _lib.call("bfhip_image_aug", cams, *tail, out.data_ptr(), _lib.stream_of(out))
        else:
            _lib.call("bfhip_image_aug_masked", cams, None if masks is None else masks.ctypes.data, *tail, out.data_ptr(),
                      _lib.stream_of(out))
        torch.cuda.synchronize()
        outs.append(out.view(torch.int16).cpu())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert not torch.isnan(outs[0].view(torch.bfloat16).float()).any()




def test_model_preprocess_with_a_mask_equals_the_torch_chain(dev, monkeypatch):
    """The camera + LiDAR model's `preprocess` (what test_step runs first) at batch 1: six raw 900 x 1600 frames with the deferred
    plan and a drawn mask record give the bits of the same call with the kernels switched off; PATHS shows which way each went."""
    from bevfusion_amd.bevfusion import nuscenes_config
    from bevfusion_amd.registry import MODELS, TRANSFORMS
    model = MODELS.build(nuscenes_config()).to(dev).eval()
    raw = np.ascontiguousarray(synthetic.camera_images_u8(1, 6, 900, 1600, seed=2000)[0].transpose(0, 2, 3, 1))
    points = [torch.from_numpy(synthetic.lidar_sweep(4000, seed=1000))]
    rig = synthetic.camera_rig(batch=1, seed=1, train_aug=False)
    data = dict(img=list(raw), ori_shape=(900, 1600), cam2img=rig["camera_intrinsics"][0], cam2lidar=rig["camera2lidar"][0])
    np.random.seed(3)
    for cfg in (dict(type="ImageAug3D", final_dim=(256, 704), resize_lim=[0.48, 0.48], bot_pct_lim=[0.0, 0.0], rot_lim=[0.0, 0.0],
                     rand_flip=False, is_train=False, defer=True),
                dict(type="GridMask", use_h=True, use_w=True, max_epoch=6, rotate=360, mode=1, prob=1.0, fixed_prob=True,
                     defer=True)):
        data = TRANSFORMS.build(cfg).transform(data)
    plan = data["img_aug_plan"]
    assert plan.grid_mask is not None and plan.grid_mask[0] == 1 and not plan[:, 5].any()
    samples = [types.SimpleNamespace(metainfo={})]
    batch = {"inputs": {"img": [torch.from_numpy(raw)], "img_aug_plan": [plan], "points": points}, "data_samples": samples}
    before = dict(ia.PATHS)
    out = model.preprocess(batch)["inputs"]["imgs"]
    assert ia.PATHS == dict(kernel=before["kernel"] + 1, torch=before["torch"])
    monkeypatch.setattr(ia, "ENABLED", False)
    ref = model.preprocess(batch)["inputs"]["imgs"]
    assert ia.PATHS == dict(kernel=before["kernel"] + 1, torch=before["torch"] + 1)
    assert out.shape == (1, 6, 3, 256, 704) and out.dtype == ref.dtype and out.stride() == ref.stride() and torch.equal(out, ref)
    masked = ia.torch_grid_mask(plan.grid_mask, 256, 704) == 0
    assert masked.any() and not masked.all() and samples[0].metainfo["batch_input_shape"] == (256, 704)
