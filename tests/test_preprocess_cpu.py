"""CPU: Det3DDataPreprocessor (bevfusion_amd/data_preprocessor.py) -- registry name, the plain-torch path against a
restatement of the reference's chain written here, validation, the state dict, the configs' mean / std and the metainfo
`preprocess()` records.  The kernel path is tests/test_preprocess_gpu.py."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bevfusion_amd  # noqa: F401
from bevfusion_amd import data_preprocessor as dp
from bevfusion_amd import synthetic
from bevfusion_amd.bevfusion import custom_data_config, nuscenes_config
from bevfusion_amd.registry import MODELS

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "custom_data_model_cfg.json")
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def oracle(imgs, mean, std, swap, divisor, pad_value):
    """Per view: channel index, .float(), (x - mean) / std; per sample: stack, F.pad bottom / right; then stack the batch."""
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


def ragged(dtype):
    g = torch.Generator().manual_seed(7)
    shapes = [(2, 3, 5, 13), (2, 3, 7, 9)]
    if dtype == torch.uint8:
        imgs = [torch.randint(0, 256, s, generator=g, dtype=torch.uint8) for s in shapes]
        for t in imgs:
            t[0, 0, 0, 0], t[1, 2, -1, -1] = 0, 255
        return imgs
    return [torch.randn(s, generator=g) * 90.0 + 20.0 for s in shapes]


def test_builds_by_registry_name():
    assert "Det3DDataPreprocessor" in MODELS
    m = MODELS.build(dict(type="Det3DDataPreprocessor", mean=MEAN, std=STD, pad_size_divisor=32, bgr_to_rgb=False,
                          voxel=True, voxelize_cfg=dict(max_num_points=10), pad_mask=False))
    assert isinstance(m, dp.Det3DDataPreprocessor) and m.pad_size_divisor == 32 and not m.swap
    assert m.mean.shape == (3, 1, 1) and m.std.shape == (3, 1, 1) and m.mean.dtype == torch.float32
    seen = {}
    target = types.SimpleNamespace(register_module=lambda name, force, module: seen.__setitem__(name, module))
    from bevfusion_amd.registry import register
    register(target)
    assert seen["Det3DDataPreprocessor"] is dp.Det3DDataPreprocessor


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("norm", [True, False])
def test_cpu_path_equals_the_oracle_on_the_ragged_batch(dtype, swap, norm):
    imgs = ragged(dtype)
    mean, std = (MEAN, STD) if norm else (None, None)
    before = dict(dp.LAUNCHES)
    for pad_value in (0, -1.5):
        want = oracle(imgs, mean, std, swap, 4, pad_value)
        assert want.shape == (2, 2, 3, 8, 16)
        m = dp.Det3DDataPreprocessor(mean=mean, std=std, pad_size_divisor=4, pad_value=pad_value, bgr_to_rgb=swap)
        out = m({"inputs": {"img": imgs}})
        assert set(out) == {"inputs", "data_samples"} and out["data_samples"] is None and set(out["inputs"]) == {"imgs"}
        assert out["inputs"]["imgs"].dtype == torch.float32 and torch.equal(out["inputs"]["imgs"], want)
        m = dp.Det3DDataPreprocessor(mean=mean, std=std, pad_size_divisor=4, pad_value=pad_value, rgb_to_bgr=swap,
                                     out_dtype=torch.bfloat16, channels_last=True)
        got = m({"inputs": {"img": imgs}})["inputs"]["imgs"]
        assert got.dtype == torch.bfloat16 and got.shape == want.shape and torch.equal(got, want.to(torch.bfloat16))
        flat = got.reshape(4, 3, 8, 16)
        assert flat.is_contiguous(memory_format=torch.channels_last) and flat.data_ptr() == got.data_ptr()
    assert dp.LAUNCHES["kernel"] == before["kernel"] and dp.LAUNCHES["torch"] == before["torch"] + 4


def test_input_forms_points_and_augmentation_list():
    m = dp.Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=8)
    g = torch.Generator().manual_seed(1)
    five = torch.randint(0, 256, (2, 3, 3, 6, 10), generator=g, dtype=torch.uint8)
    want = oracle(list(five), MEAN, STD, False, 8, 0)
    pts = [torch.randn(5, 4), torch.randn(7, 4)]
    out = m({"inputs": {"img": five, "points": pts}, "data_samples": None})
    assert torch.equal(out["inputs"]["imgs"], want) and out["inputs"]["points"][1] is pts[1]
    # 3-D list / 4-D tensor: one view
    single = oracle([t[:1] for t in five], MEAN, STD, False, 8, 0)
    assert torch.equal(m({"inputs": {"img": [t[0] for t in five]}})["inputs"]["imgs"], single)
    assert torch.equal(m({"inputs": {"img": five[:, 0]}})["inputs"]["imgs"], single)
    # no image, no points
    assert m({"inputs": {"points": pts}})["inputs"].keys() == {"points"}
    assert m({"inputs": {"img": five}})["inputs"].keys() == {"imgs"}
    # test-time augmentation: a list of batches, one at a time
    outs = m([{"inputs": {"img": five}}, {"inputs": {"img": five.flip(-1)}}])
    assert isinstance(outs, list) and len(outs) == 2 and torch.equal(outs[0]["inputs"]["imgs"], want)
    assert torch.equal(outs[1]["inputs"]["imgs"], oracle(list(five.flip(-1)), MEAN, STD, False, 8, 0))
    # one-value mean and other dtypes take the torch path
    one = dp.Det3DDataPreprocessor(mean=[100.0], std=[50.0])
    assert torch.equal(one({"inputs": {"img": five}})["inputs"]["imgs"], oracle(list(five), [100.0], [50.0], False, 1, 0))
    half = dp.Det3DDataPreprocessor()({"inputs": {"img": five.to(torch.int16)}})["inputs"]["imgs"]
    assert half.dtype == torch.float32 and torch.equal(half, five.float())


def test_validation_errors():
    with pytest.raises(ValueError, match="together"):
        dp.Det3DDataPreprocessor(mean=MEAN)
    with pytest.raises(ValueError, match="together"):
        dp.Det3DDataPreprocessor(std=STD)
    with pytest.raises(ValueError, match="3 values"):
        dp.Det3DDataPreprocessor(mean=[1.0, 2.0], std=[1.0, 2.0])
    with pytest.raises(ValueError, match="3 values"):
        dp.Det3DDataPreprocessor(mean=MEAN, std=[1.0])
    with pytest.raises(ValueError, match="both"):
        dp.Det3DDataPreprocessor(bgr_to_rgb=True, rgb_to_bgr=True)
    with pytest.raises(ValueError, match="pad_mask"):
        dp.Det3DDataPreprocessor(pad_mask=True)
    with pytest.raises(TypeError, match="unknown"):
        dp.Det3DDataPreprocessor(no_such_keyword=1)
    with pytest.raises(ValueError, match="out_dtype"):
        dp.Det3DDataPreprocessor(out_dtype=torch.float16)
    m = dp.Det3DDataPreprocessor()
    with pytest.raises(ValueError, match="views"):
        m({"inputs": {"img": [torch.zeros(2, 3, 4, 4), torch.zeros(3, 3, 4, 4)]}})


def test_entry_point_rejects_bad_arguments_on_the_host():
    """bfhip_img_preprocess validates before it launches: a padded size below a sample's own size, an unknown dtype and a
    missing mean are BFHIP_E_INVALID without touching a device."""
    import ctypes
    from bevfusion_amd import _lib
    lib = _lib.load()
    assert lib.bfhip_img_preprocess_max_samples() >= 1
    descs = (_lib.ImgDesc * 1)(_lib.ImgDesc(0x1000, 5, 13))
    mean, std = _lib.host_f32(MEAN), _lib.host_f32(STD)
    call = lambda **kw: lib.bfhip_img_preprocess(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("descs", descs), ("n", 1), ("views", 2), ("src", 0), ("swap", 0), ("norm", 1), ("mean", mean), ("std", std),
        ("pad", 0.0), ("Hp", 8), ("Wp", 16), ("out_dtype", 0), ("pix", 0), ("out", 0x2000), ("stream", None))])
    assert call(Hp=4) == -1 and b"larger than the padded" in lib.bfhip_last_error()
    assert call(Wp=12) == -1
    assert call(src=2) == -1 and call(out_dtype=3) == -1 and call(views=0) == -1 and call(n=0) == -1
    assert call(mean=None) == -1 and call(out=None) == -1
    assert call(descs=(_lib.ImgDesc * 1)(_lib.ImgDesc(None, 5, 13))) == -1
    assert ctypes.sizeof(_lib.ImgDesc) == 16


def test_buffers_stay_out_of_the_state_dict():
    m = dp.Det3DDataPreprocessor(mean=MEAN, std=STD)
    assert len(m.state_dict()) == 0 and {n for n, _ in m.named_buffers()} >= {"mean", "std"}
    model = MODELS.build(nuscenes_config())
    assert isinstance(model.data_preprocessor, dp.Det3DDataPreprocessor)
    assert model.data_preprocessor.pad_size_divisor == 32 and model.data_preprocessor.mean is not None
    keys = list(model.state_dict())
    assert not any(k.startswith("data_preprocessor") for k in keys)
    # exactly the keys of the other children: what the model had before it owned a preprocessor
    others = [n + "." + k for n, c in model.named_children() if n != "data_preprocessor" for k in c.state_dict()]
    assert keys == others
    # a dict without mean only casts and stacks
    plain = MODELS.build(nuscenes_config(camera=False)).data_preprocessor
    assert plain.mean is None and plain.std is None


def test_configs_carry_the_reference_mean_and_std():
    with open(GOLDEN) as f:
        ref = json.load(f)["data_preprocessor"]
    assert ref["mean"] == MEAN and ref["std"] == STD
    for cfg in (nuscenes_config(), custom_data_config()):
        pre = cfg["data_preprocessor"]
        assert pre["mean"] == ref["mean"] and pre["std"] == ref["std"]
        assert pre["bgr_to_rgb"] is ref["bgr_to_rgb"] is False and pre["pad_size_divisor"] == ref["pad_size_divisor"] == 32
        assert "voxelize_cfg" in pre
    for cfg in (nuscenes_config(camera=False), custom_data_config(camera=False)):
        assert "mean" not in cfg["data_preprocessor"] and "std" not in cfg["data_preprocessor"]


class _Sample:
    def __init__(self, **meta):
        self.metainfo = dict(meta)


class _SetSample:
    def __init__(self):
        self.info = {}

    def set_metainfo(self, info):
        self.info.update(info)


def test_preprocess_records_the_padded_shapes():
    model = MODELS.build(nuscenes_config(camera=False))
    model.data_preprocessor = dp.Det3DDataPreprocessor(mean=MEAN, std=STD, pad_size_divisor=32)
    imgs = [torch.zeros(2, 3, 30, 70, dtype=torch.uint8), torch.zeros(2, 3, 40, 60, dtype=torch.uint8)]
    samples = [_Sample(token="a"), _SetSample(), ]
    out = model.preprocess({"inputs": {"img": imgs, "points": [torch.zeros(3, 5), torch.zeros(4, 5)]},
                            "data_samples": samples})
    assert out["inputs"]["imgs"].shape == (2, 2, 3, 64, 96) and out["data_samples"] is not None
    assert out["data_samples"][0].metainfo == dict(token="a", batch_input_shape=(64, 96), pad_shape=(32, 96))
    assert out["data_samples"][1].info == dict(batch_input_shape=(64, 96), pad_shape=(64, 64))
    assert callable(model.test_step) and callable(model.val_step)


def test_camera_images_u8_is_seeded_and_full_range():
    a = synthetic.camera_images_u8(2, 3, 16, 24, seed=5)
    assert a.shape == (2, 3, 3, 16, 24) and a.dtype == np.uint8
    assert np.array_equal(a, synthetic.camera_images_u8(2, 3, 16, 24, seed=5))
    assert not np.array_equal(a, synthetic.camera_images_u8(2, 3, 16, 24, seed=6))
    big = synthetic.camera_images_u8(1, 6, 64, 96)
    assert big.min() == 0 and big.max() == 255 and 60 < big.mean() < 190
