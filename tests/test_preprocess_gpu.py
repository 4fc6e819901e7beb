"""GPU: csrc/preprocess.hip (bfhip_img_preprocess) through Det3DDataPreprocessor and through the C entry point.

The oracle is the reference's chain restated in torch and run on the CPU: per view channel index, .float(), (x - mean) / std;
per sample stack and F.pad at the bottom and right; then the batch stack.  The bf16 expectation is that result
.to(torch.bfloat16).  The kernel's arithmetic is the same fp32 operations in the same order (true division), so every
comparison is torch.equal: no tolerance applies."""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, synthetic
from bevfusion_amd import data_preprocessor as dp

pytestmark = pytest.mark.gpu
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
FORMS = [(None, False), (None, True), (torch.bfloat16, False), (torch.bfloat16, True)]  # (out_dtype, channels_last)
FORM_IDS = ["f32", "f32-cl", "bf16", "bf16-cl"]


def oracle(imgs, mean, std, swap, divisor, pad_value):
    Hp = -(-max(t.shape[-2] for t in imgs) // divisor) * divisor
    Wp = -(-max(t.shape[-1] for t in imgs) // divisor) * divisor
    m = None if mean is None else torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
    s = None if std is None else torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)
    batch = []
    for sample in imgs:
        views = []
        for v in sample:
            v = v[[2, 1, 0], ...] if swap else v
            v = v.float()
            views.append(v if m is None else (v - m) / s)
        x = torch.stack(views)
        batch.append(F.pad(x, (0, Wp - x.shape[-1], 0, Hp - x.shape[-2]), "constant", pad_value))
    return torch.stack(batch)


def make(shapes, dtype, seed=7):
    """Seeded CPU inputs: uint8 with 0 and 255 present; float32 with non-integers and negatives (a kernel that routes floats
    through bytes fails on them)."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        imgs = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in shapes]
        for t in imgs:
            t.view(-1)[0], t.view(-1)[-1] = 0, 255
        return imgs
    imgs = [torch.randn(s, generator=g) * 90.0 + 20.0 for s in shapes]
    assert all((t < 0).any() and (t != t.round()).any() for t in imgs)
    return imgs


def run(imgs, dev, kernel=True, **kw):
    """The module on `dev` -> imgs on the CPU; asserts which path took the batch."""
    m = dp.Det3DDataPreprocessor(**kw).to(dev)
    before = dict(dp.LAUNCHES)
    out = m({"inputs": {"img": imgs}})["inputs"]["imgs"]
    took = {k: dp.LAUNCHES[k] - before[k] for k in before}
    assert took == (dict(kernel=1, torch=0) if kernel else dict(kernel=0, torch=1)), took
    assert out.is_cuda
    if kw.get("channels_last"):
        B, N, C, H, W = out.shape
        flat = out.reshape(B * N, C, H, W)
        assert flat.is_contiguous(memory_format=torch.channels_last) and flat.data_ptr() == out.data_ptr()
    else:
        assert out.is_contiguous()
    return out.cpu()


RAGGED = {dt: make([(2, 3, 5, 13), (2, 3, 7, 9)], dt) for dt in (torch.uint8, torch.float32)}
_ragged_want = {}


def ragged_want(dtype, swap, norm, pad_value):
    key = (dtype, swap, norm, pad_value)
    if key not in _ragged_want:
        _ragged_want[key] = oracle(RAGGED[dtype], MEAN if norm else None, STD if norm else None, swap, 4, pad_value)
    return _ragged_want[key]


@pytest.mark.parametrize("pad_value", [0, -1.5])
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("swap", [False, True], ids=["rgb", "swap"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_ragged_small_batch(dev, dtype, form, swap, norm, pad_value):
    want = ragged_want(dtype, swap, norm, pad_value)
    assert want.shape == (2, 2, 3, 8, 16)
    out = run(RAGGED[dtype], dev, mean=MEAN if norm else None, std=STD if norm else None, pad_size_divisor=4,
              pad_value=pad_value, bgr_to_rgb=swap, out_dtype=form[0], channels_last=form[1])
    assert out.dtype == (form[0] or torch.float32)
    assert torch.equal(out, want if form[0] is None else want.to(form[0]))


def _offset_source(t, dev):
    """t on the device with its storage starting one ELEMENT into an allocation: contiguous, but not vector-aligned."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % (8 if t.dtype == torch.uint8 else 16) != 0
    return view


VECTOR_CASES = [  # (name, sample shapes, divisor, padded size, offset source)
    ("aligned rows, padded below", [(6, 3, 8, 64)], 32, (32, 64), False),
    ("width a multiple of 8, padded right", [(1, 3, 9, 72)], 32, (32, 96), False),
    ("odd width, no padding", [(1, 3, 4, 67)], 1, (4, 67), False),
    ("source one element into its allocation", [(2, 3, 8, 64)], 32, (32, 64), True),
    ("two samples, one narrower by a partial run", [(2, 3, 8, 64), (2, 3, 6, 52)], 32, (32, 64), False),
]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("case", VECTOR_CASES, ids=[c[0] for c in VECTOR_CASES])
def test_vector_path_and_its_edges(dev, case, dtype, form):
    _, shapes, divisor, padded, offset = case
    imgs = make(shapes, dtype, seed=11)
    want = oracle(imgs, MEAN, STD, True, divisor, 3.25)
    assert tuple(want.shape[-2:]) == padded
    src = [_offset_source(t, dev) for t in imgs] if offset else imgs
    out = run(src, dev, mean=MEAN, std=STD, pad_size_divisor=divisor, pad_value=3.25, bgr_to_rgb=True, out_dtype=form[0],
              channels_last=form[1])
    assert torch.equal(out, want if form[0] is None else want.to(form[0]))


@pytest.mark.parametrize("margin", [64, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_element_written_once_nothing_outside(dev, form, margin):
    """The C entry point writes into the middle of a buffer filled with a NaN bit pattern that neither the inputs (finite)
    nor pad_value can produce (the kernel's bf16 conversion only ever makes the canonical 0x7fc0 NaN): the margins keep it,
    no output element does.  margin 3 elements: an output that is not 16-byte aligned (element-wise stores)."""
    out_dtype, pixel_major = form
    bf16 = out_dtype == torch.bfloat16
    imgs = [t.to(dev) for t in make([(2, 3, 5, 13), (2, 3, 8, 16), (2, 3, 7, 9)], torch.uint8, seed=3)]
    want = oracle([t.cpu() for t in imgs], MEAN, STD, False, 8, -2.0)
    B, N, _, Hp, Wp = want.shape
    n = want.numel()
    bits, sentinel = (torch.int16, 0x7fc1) if bf16 else (torch.int32, 0x7fc12345)
    buf = torch.full((margin + n + margin,), sentinel, dtype=bits, device=dev)
    inner = buf[margin:margin + n]
    assert (inner.data_ptr() % 16 == 0) == (margin == 64)
    descs = (_lib.ImgDesc * B)(*[_lib.ImgDesc(t.data_ptr(), t.shape[2], t.shape[3]) for t in imgs])
    _lib.call("bfhip_img_preprocess", descs, B, N, 0, 0, 1, _lib.host_f32(MEAN), _lib.host_f32(STD), -2.0, Hp, Wp, int(bf16),
              int(pixel_major), inner.data_ptr(), _lib.stream_of(buf))
    torch.cuda.synchronize()
    assert (buf[:margin] == sentinel).all() and (buf[margin + n:] == sentinel).all()
    assert not (inner == sentinel).any()
    got = inner.view(torch.bfloat16 if bf16 else torch.float32)
    got = got.view(B * N, Hp, Wp, 3).permute(0, 3, 1, 2).reshape(B, N, 3, Hp, Wp) if pixel_major else got.view(B, N, 3, Hp, Wp)
    assert torch.equal(got.cpu(), want.to(torch.bfloat16) if bf16 else want)


@pytest.mark.parametrize("form", [FORMS[0], FORMS[3]], ids=[FORM_IDS[0], FORM_IDS[3]])
def test_more_samples_than_one_launch_holds(dev, form):
    n = _lib.load().bfhip_img_preprocess_max_samples() + 1
    imgs = make([(1, 3, 2, 2)] * n, torch.uint8, seed=5)
    want = oracle(imgs, MEAN, STD, False, 1, 0)
    assert want.shape == (n, 1, 3, 2, 2)
    out = run(imgs, dev, mean=MEAN, std=STD, out_dtype=form[0], channels_last=form[1])
    assert torch.equal(out, want if form[0] is None else want.to(form[0]))


@pytest.fixture
def reproducible_library(monkeypatch):
    """The library convolutions (MIOpen through torch: the ResNet-50 stem and, in eval mode, its trunk) pick solvers that
    accumulate with atomics: the SAME tensor through the SAME eval-mode ResNet50 on [2, 3, 32, 64] differed run to run (none of
    five repeats equalled the first; between two calls 62 of the 32768 elements of layer2.0, the first layer to differ), and
    so did BEVFusion.predict at batch 1.  With the deterministic solvers every repeat of both was bit-identical, so a bit
    comparison of two forwards asks the library for them."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)


def test_channels_last_batch_feeds_resnet_without_a_cast(dev, reproducible_library):
    """Under bf16 autocast ResNet50 gives the same bits for the preprocessor's bf16 channels-last batch (its own cast pass
    skipped) and for the oracle's fp32 batch."""
    from bevfusion_amd.dense_modules import ResNet50
    imgs = make([(1, 3, 32, 64), (1, 3, 32, 64)], torch.uint8, seed=13)
    want = oracle(imgs, MEAN, STD, False, 32, 0)
    m = dp.Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=32, out_dtype=torch.bfloat16, channels_last=True).to(dev)
    batch = m({"inputs": {"img": imgs}})["inputs"]["imgs"]
    x = batch.reshape(2, 3, 32, 64)
    assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() == batch.data_ptr()
    torch.manual_seed(0)
    net = ResNet50().to(dev).eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        a = net(x)
        b = net(want.reshape(2, 3, 32, 64).to(dev))
    assert len(a) == len(b) == 3
    for u, v in zip(a, b):
        assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v)


def test_switch_off_gives_the_same_bits_through_torch(dev, monkeypatch):
    monkeypatch.setattr(dp, "ENABLED", False)
    for dtype in (torch.uint8, torch.float32):
        for form in FORMS:
            want = ragged_want(dtype, True, True, -1.5)
            out = run(RAGGED[dtype], dev, kernel=False, mean=MEAN, std=STD, pad_size_divisor=4, pad_value=-1.5, rgb_to_bgr=True,
                      out_dtype=form[0], channels_last=form[1])
            assert torch.equal(out, want if form[0] is None else want.to(form[0]))
    # what the kernel does not take goes the same way with the switch on
    monkeypatch.setattr(dp, "ENABLED", True)
    strided = [t.to(dev).transpose(-1, -2).contiguous().transpose(-1, -2) for t in RAGGED[torch.uint8]]
    assert not strided[0].is_contiguous()
    assert torch.equal(run(strided, dev, kernel=False, mean=MEAN, std=STD, pad_size_divisor=4),
                       ragged_want(torch.uint8, False, True, 0))


def test_test_step_equals_predict_on_the_oracle_batch(dev, reproducible_library):
    """Camera + LiDAR model (the nuScenes dict at batch 1, the size tests/test_model_gpu.py uses): test_step() on raw uint8
    frames returns the boxes, scores and labels of predict() fed the oracle-normalised tensor -- with the reference's fp32
    batch and with the bf16 channels-last batch the backbone reads without a cast."""
    from bevfusion_amd.bevfusion import nuscenes_config
    from bevfusion_amd.registry import MODELS
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config()).to(dev).eval()
    frames = torch.from_numpy(synthetic.camera_images_u8(1, 6, 256, 704, seed=2000))
    points = [torch.from_numpy(synthetic.lidar_sweep(40000, seed=1000))]
    rig = synthetic.camera_rig(batch=1, seed=1, train_aug=False)
    meta = {dst: rig[src][0] for src, dst in (("lidar2image", "lidar2img"), ("camera_intrinsics", "cam2img"),
                                               ("camera2lidar", "cam2lidar"), ("img_aug_matrix", "img_aug_matrix"),
                                               ("lidar_aug_matrix", "lidar_aug_matrix"))}
    samples = [types.SimpleNamespace(metainfo=dict(meta))]
    want = oracle(list(frames), MEAN, STD, False, 32, 0)
    assert want.shape == (1, 6, 3, 256, 704)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = model.predict({"points": [p.to(dev) for p in points], "imgs": want.to(dev)}, samples)
        outs = []
        for out_dtype, channels_last in (FORMS[0], FORMS[3]):
            model.data_preprocessor.out_dtype, model.data_preprocessor.channels_last = out_dtype, channels_last
            before = dp.LAUNCHES["kernel"]
            outs.append(model.test_step({"inputs": {"img": list(frames), "points": points}, "data_samples": samples}))
            assert dp.LAUNCHES["kernel"] == before + 1
        val = model.val_step({"inputs": {"img": frames, "points": points}, "data_samples": samples})
    assert samples[0].metainfo["batch_input_shape"] == (256, 704) and samples[0].metainfo["pad_shape"] == (256, 704)
    assert len(ref) == 1 and ref[0]["bboxes_3d"].shape[0] > 0
    for out in outs + [val]:
        assert len(out) == 1
        for key in ("bboxes_3d", "scores_3d", "labels_3d"):
            assert torch.equal(out[0][key], ref[0][key]), key


def test_entry_point_rejects_a_padded_size_below_a_sample(dev):
    t = torch.zeros(1, 3, 5, 13, dtype=torch.uint8, device=dev)
    out = torch.zeros(3 * 8 * 16, device=dev)
    descs = (_lib.ImgDesc * 1)(_lib.ImgDesc(t.data_ptr(), 5, 13))
    for Hp, Wp in ((4, 16), (8, 12)):
        with pytest.raises(RuntimeError, match="larger than the padded"):
            _lib.call("bfhip_img_preprocess", descs, 1, 1, 0, 0, 0, None, None, 0.0, Hp, Wp, 0, 0, out.data_ptr(),
                      _lib.stream_of(out))
    assert ctypes.sizeof(_lib.ImgDesc) == 16 and np.dtype(np.uint8).itemsize == 1
