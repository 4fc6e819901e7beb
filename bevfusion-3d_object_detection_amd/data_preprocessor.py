"""Det3DDataPreprocessor: what stands between the data pipeline and the model (mmdet3d's
M3D/models/data_preprocessors/data_preprocessor.py:126-330 on mmengine's ImgDataPreprocessor): move the batch to the device,
swap the image channels, normalise, pad to the size divisor at the bottom and right and stack the per-sample
[N, 3, h, w] camera blocks into `imgs` [B, N, 3, H', W'].  Points pass through (BEVFusion voxelizes them itself,
BF/bevfusion.py:45).

On the GPU the image path is ONE kernel (csrc/preprocess.hip, bfhip_img_preprocess): it reads the raw uint8 / float32 pixels
once and writes the batch once, optionally already in bf16 and pixel-major (`out_dtype`, `channels_last`: this package's
own keywords) -- the form ResNet50.forward would otherwise make with one more pass.  The arithmetic is the reference's,
(float(x) - mean) / std in fp32 with a true division, so both paths give the same bits.

`inputs["img_aug_plan"]` (image_aug.ImageAug3D(defer=True)): `img` then holds the RAW uint8 frames [N, H, W, 3] per sample and the
resize / crop / flip / rotate of ImageAug3D runs on the device in front of the same stores (`process_frames`, csrc/image_aug.hip;
BFHIP_IMG_AUG=0 or a CPU batch: image_aug.torch_image_aug, then the path below).  A plan that carries a GridMask record
(image_aug.GridMask(defer=True): `plan.grid_mask`) has that mask applied on either path, after the frame's own flip and rotation
and before normalise and pad.

`inputs["points_aug_plan"]` (the point transforms of points_aug.py with defer=True): `points` then holds the loaded points and the
rotate / scale / translate, flips, range filter and shuffle of the plans run on the device (`process_points`, csrc/points_aug.hip;
BFHIP_POINTS_AUG=0 or a CPU batch: points_aug.torch_points_aug, same bits).  Without a plan points pass through as they are.

A sample of `img` that is a jpeg.JpegFrames (loading.BEVLoadMultiViewImageFromFiles(defer=True): entropy-decoded JPEG frames)
is first decoded on the device into that raw uint8 [N, H, W, 3] block (`decode_jpeg`, csrc/jpeg.hip: one pinned upload and two
launches for the batch; BFHIP_JPEG_DECODE=0 or a CPU module: jpeg.torch_jpeg_decode, same bits), then goes on as above: through
`process_frames` with a plan, otherwise through `process_imgs` on its [N, 3, H, W] view.

BFHIP_IMG_PREPROCESS (ships on; measured: DESIGN.md section 6): 0 selects the plain-torch restatement below, which also
serves whatever the kernel does not take -- CPU tensors, other dtypes, non-contiguous blocks, a one-value mean.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .registry import MODELS

ENABLED = os.environ.get("BFHIP_IMG_PREPROCESS", "1") != "0"
LAUNCHES = {"kernel": 0, "torch": 0}  # image batches taken by each path (tests, tools)

# reference keywords without a counterpart here: accepted at the value that makes them a no-op, an error otherwise
_NOOP_DEFAULTS = dict(pad_mask=False, pad_seg=False, batch_augments=None, boxtype2tensor=True)
# accepted and ignored: BEVFusion pops the voxelization itself; the two pad values only matter with pad_mask / pad_seg
_IGNORED = ("voxel", "voxel_type", "voxel_layer", "batch_first", "max_voxels", "voxelize_cfg", "voxelize_reduce",
            "mask_pad_value", "seg_pad_value")


def round_up(v, divisor):
    return (int(v) + divisor - 1) // divisor * divisor


def torch_preprocess(imgs, mean=None, std=None, swap=False, pad_size_divisor=1, pad_value=0):
    """The reference's chain in plain torch.  imgs: list of [N, 3, h, w]; mean / std: tensors [C, 1, 1] or None.
    Per view: channel index, .float(), (x - mean) / std; per sample: stack, F.pad at the bottom and right; then the batch
    stack -> fp32 [B, N, 3, H', W']."""
    Hp = round_up(max(t.shape[-2] for t in imgs), pad_size_divisor)
    Wp = round_up(max(t.shape[-1] for t in imgs), pad_size_divisor)
    batch = []
    for sample in imgs:
        views = []
        for x in sample:
            if swap:
                x = x[[2, 1, 0], ...]
            x = x.float()
            if mean is not None:
                x = (x - mean) / std
            views.append(x)
        x = torch.stack(views, 0)
        batch.append(F.pad(x, (0, Wp - x.shape[-1], 0, Hp - x.shape[-2]), "constant", pad_value))
    return torch.stack(batch, 0)


def _pixel_major(x):
    """[B, N, 3, H, W] with the same logical shape and pixel-major strides: x.reshape(B * N, 3, H, W) is then a
    torch.channels_last view."""
    B, N, C, H, W = x.shape
    return x.reshape(B * N, C, H, W).contiguous(memory_format=torch.channels_last).view(B, N, C, H, W)


@MODELS.register_module()
class Det3DDataPreprocessor(nn.Module):
    """forward(data, training=False): data = {"inputs": {"points": [...], "img": [...]}, "data_samples": [...] or None} (or a
    list of such dicts: test-time augmentation, one at a time) -> {"inputs": {"points": [...], "imgs": Tensor[B, N, 3, H', W']},
    "data_samples": ...}.  `img`: a list of [N, 3, h, w] tensors (uint8 or float32 raw pixel values; h and w may differ), or
    a [B, N, 3, H, W] tensor; a list of [3, h, w] tensors or a [B, 3, H, W] tensor is N = 1.

    out_dtype: None / torch.float32 as the reference, or torch.bfloat16.  channels_last: `imgs` keeps its logical shape and
    gets pixel-major strides, so that BEVFusion.extract_img_feat's reshape(B * N, 3, H', W') is a torch.channels_last view
    without a copy and ResNet50.forward (bf16 input) skips its own cast pass."""

    def __init__(self, mean=None, std=None, pad_size_divisor=1, pad_value=0, bgr_to_rgb=False, rgb_to_bgr=False,
                 non_blocking=False, out_dtype=None, channels_last=False, **kwargs):
        super().__init__()
        for key, value in kwargs.items():
            if key in _IGNORED:
                continue
            if key not in _NOOP_DEFAULTS:
                raise TypeError("Det3DDataPreprocessor: unknown keyword %r" % key)
            if value != _NOOP_DEFAULTS[key]:
                raise ValueError("Det3DDataPreprocessor: %s=%r is not supported (only %r)" % (key, value, _NOOP_DEFAULTS[key]))
        if (mean is None) != (std is None):
            raise ValueError("mean and std must be given together")
        if bgr_to_rgb and rgb_to_bgr:
            raise ValueError("bgr_to_rgb and rgb_to_bgr cannot both be set")
        if mean is not None:
            if len(mean) != len(std) or len(mean) not in (1, 3):
                raise ValueError("mean and std must have 3 values each (or 1), got %d and %d" % (len(mean), len(std)))
            # [C, 1, 1] fp32 buffers outside the state dict, as mmengine's ImgDataPreprocessor registers them
            self.register_buffer("mean", torch.tensor([float(v) for v in mean], dtype=torch.float32).view(-1, 1, 1), False)
            self.register_buffer("std", torch.tensor([float(v) for v in std], dtype=torch.float32).view(-1, 1, 1), False)
            self._mean_std = (tuple(float(v) for v in mean), tuple(float(v) for v in std))  # the kernel takes them by value
        else:
            self.mean = self.std = None
        if out_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("out_dtype must be None, torch.float32 or torch.bfloat16, got %r" % (out_dtype,))
        if int(pad_size_divisor) < 1:
            raise ValueError("pad_size_divisor must be positive, got %r" % (pad_size_divisor,))
        self.pad_size_divisor = int(pad_size_divisor)
        self.pad_value = pad_value
        self.swap = bool(bgr_to_rgb or rgb_to_bgr)
        self.non_blocking = bool(non_blocking)
        self.out_dtype = out_dtype
        self.channels_last = bool(channels_last)
        self.register_buffer("_anchor", torch.empty(0), False)  # follows .to() / .cuda(): where the batch goes

    @property
    def device(self):
        return self._anchor.device

    # ------------------------------------------------------------------ batch plumbing
    def cast_data(self, data):
        """Every tensor of a nested dict / list moved to the module's device (mmengine's BaseDataPreprocessor.cast_data)."""
        if torch.is_tensor(data):
            return data.to(self.device, non_blocking=self.non_blocking)
        if isinstance(data, dict):
            return {k: self.cast_data(v) for k, v in data.items()}
        if isinstance(data, (list, tuple)):
            return [self.cast_data(v) for v in data]
        if not isinstance(data, (str, bytes, nn.Module)) and callable(getattr(data, "to", None)):
            return data.to(self.device)  # a data sample that knows how to move itself
        return data

    @staticmethod
    def _sample_list(img):
        """`img` as the list of [N, 3, h, w] blocks."""
        if torch.is_tensor(img):
            if img.dim() == 5:
                return list(img.unbind(0))
            if img.dim() == 4:
                return [t.unsqueeze(0) for t in img.unbind(0)]
            raise ValueError("img must be [B, N, 3, H, W] or [B, 3, H, W], got %s" % (tuple(img.shape),))
        img = list(img)
        if not img or not all(torch.is_tensor(t) for t in img):
            raise TypeError("img must be a tensor or a non-empty list of tensors")
        if img[0].dim() == 3:
            img = [t.unsqueeze(0) for t in img]
        if any(t.dim() != 4 for t in img):
            raise ValueError("every sample of img must be [N, 3, h, w] (or every one [3, h, w])")
        if any(t.shape[0] != img[0].shape[0] for t in img):
            raise ValueError("every sample must have the same number of views, got %s" % [int(t.shape[0]) for t in img])
        return img

    def _takes_kernel(self, imgs):
        first = imgs[0]
        return (ENABLED and first.is_cuda and first.dtype in (torch.uint8, torch.float32)
                and (self.mean is None or self.mean.shape[0] == 3)
                and all(t.is_cuda and t.device == first.device and t.dtype == first.dtype and t.shape[1] == 3
                        and t.is_contiguous() for t in imgs))

    def process_imgs(self, imgs):
        """list of [N, 3, h, w] on the module's device -> imgs [B, N, 3, H', W'] in out_dtype / the requested strides."""
        Hp = round_up(max(t.shape[-2] for t in imgs), self.pad_size_divisor)
        Wp = round_up(max(t.shape[-1] for t in imgs), self.pad_size_divisor)
        if self._takes_kernel(imgs):
            LAUNCHES["kernel"] += 1
            return self._kernel(imgs, Hp, Wp)
        LAUNCHES["torch"] += 1
        x = torch_preprocess(imgs, self.mean, self.std, self.swap, self.pad_size_divisor, self.pad_value)
        if self.out_dtype is not None:
            x = x.to(self.out_dtype)
        return _pixel_major(x) if self.channels_last else x

    def _kernel(self, imgs, Hp, Wp):
        B, N, dev = len(imgs), imgs[0].shape[0], imgs[0].device
        dtype = torch.bfloat16 if self.out_dtype == torch.bfloat16 else torch.float32
        if self.channels_last:
            store = torch.empty((B * N, Hp, Wp, 3), dtype=dtype, device=dev)
            out = store.permute(0, 3, 1, 2).view(B, N, 3, Hp, Wp)
        else:
            out = store = torch.empty((B, N, 3, Hp, Wp), dtype=dtype, device=dev)
        descs = (_lib.ImgDesc * B)(*[_lib.ImgDesc(t.data_ptr(), t.shape[2], t.shape[3]) for t in imgs])
        normalise = self.mean is not None
        mean, std = (_lib.host_f32(v) for v in self._mean_std) if normalise else (None, None)
        with torch.cuda.device(dev):
            _lib.call("bfhip_img_preprocess", descs, B, N,
                      0 if imgs[0].dtype == torch.uint8 else 1, int(self.swap), int(normalise),
                      mean, std, float(self.pad_value), Hp, Wp,
                      1 if dtype == torch.bfloat16 else 0, int(self.channels_last), store.data_ptr(), _lib.stream_of(store))
        return out

    def process_frames(self, frames, plans):
        """Deferred ImageAug3D: frames = per sample the raw uint8 [N, H, W, 3] block (a list, or one [B, N, H, W, 3] tensor),
        plans = per sample the AugPlan of image_aug.ImageAug3D(defer=True) -> the bits of
        process_imgs([torch_image_aug(f, p) for f, p in zip(frames, plans)]), on the GPU through csrc/image_aug.hip."""
        from . import image_aug
        frames = list(frames.unbind(0)) if torch.is_tensor(frames) else list(frames)
        plans = [plans] if hasattr(plans, "ndim") and plans.ndim == 2 else list(plans)
        if len(frames) != len(plans) or not frames:
            raise ValueError("img_aug_plan: %d plans for %d samples" % (len(plans), len(frames)))
        dims = {getattr(p, "final_dim", None) for p in plans}
        if len(dims) != 1 or None in dims:
            raise ValueError("img_aug_plan: every sample needs an AugPlan with one final_dim, got %s" % sorted(map(str, dims)))
        if (image_aug.ENABLED and (self.mean is None or self.mean.shape[0] == 3)
                and all(torch.is_tensor(f) and f.dim() == 4 and len(p) == f.shape[0] for f, p in zip(frames, plans))
                and image_aug.fused_supported(frames, plans)):
            image_aug.PATHS["kernel"] += 1
            return image_aug.fused_image_aug(frames, plans, None, self._mean_std if self.mean is not None else None, self.swap,
                                             self.pad_size_divisor, self.pad_value, self.out_dtype, self.channels_last)
        image_aug.PATHS["torch"] += 1
        return self.process_imgs([image_aug.torch_image_aug(f, p) for f, p in zip(frames, plans)])

    def decode_jpeg(self, img, planar):
        """The JpegFrames samples of `img` decoded into uint8 [N, H, W, 3] blocks on the module's device, all in one batch (a
        numpy uint8 [N, H, W, 3] block -- a sample the loader decoded on the host -- is moved there); with `planar` those
        blocks as their [N, 3, H, W] views.  Anything else is returned as it came."""
        from . import jpeg
        if isinstance(img, jpeg.JpegFrames):
            img = [img]
        if not isinstance(img, (list, tuple)):
            return img
        img = list(img)
        raw = [i for i, s in enumerate(img) if isinstance(s, np.ndarray) and s.dtype == np.uint8 and s.ndim == 4 and s.shape[-1] == 3]
        deferred = [i for i, s in enumerate(img) if isinstance(s, jpeg.JpegFrames)]
        for i in raw:
            img[i] = torch.from_numpy(img[i]).to(self.device)
        if deferred:
            for i, block in zip(deferred, jpeg.decode_frames([img[i] for i in deferred], self.device)):
                img[i] = block
        if planar:
            for i in raw + deferred:
                img[i] = img[i].permute(0, 3, 1, 2)
        return img

    def process_points(self, points, plans):
        """Deferred GlobalRotScaleTrans / RandomFlip3D / PointsRangeFilter / PointShuffle: points = per sample the loaded
        [n, C] tensor, plans = per sample the PointsAugPlan the transforms wrote with defer=True -> the list of float32
        [kept, C] tensors, views of one buffer, the bits of points_aug.torch_points_aug per sample.  On the GPU through
        csrc/points_aug.hip; the views' shapes need the B kept counts on the host, read with ONE host read per batch."""
        from . import points_aug
        return points_aug.process_points(points, plans)

    # ------------------------------------------------------------------ the reference's entry points
    def forward(self, data, training=False):
        if isinstance(data, (list, tuple)):  # test-time augmentation: one batch dict per augmentation
            return [self.simple_process(d, training) for d in data]
        return self.simple_process(data, training)

    def simple_process(self, data, training=False):
        data = self.cast_data(data)
        inputs, samples = data["inputs"], data.get("data_samples")
        batch_inputs = {}
        if "points" in inputs:
            if inputs.get("points_aug_plan") is not None:  # the deferred point transforms' plans: augment on the device
                batch_inputs["points"] = self.process_points(inputs["points"], inputs["points_aug_plan"])
            else:
                batch_inputs["points"] = inputs["points"]
        if "img" in inputs:
            # entropy-decoded JPEG frames first become the raw blocks: [N, H, W, 3] for a plan, [N, 3, H, W] views without one
            inputs = dict(inputs, img=self.decode_jpeg(inputs["img"], planar=inputs.get("img_aug_plan") is None))
            if inputs.get("img_aug_plan") is not None:  # raw frames + ImageAug3D(defer=True)'s plans: augment on the device
                batch = self.process_frames(inputs["img"], inputs["img_aug_plan"])
                sizes = [batch.shape[-2:]] * batch.shape[0]  # every sample is final_dim, padded to the divisor
            else:
                imgs = self._sample_list(inputs["img"])
                batch = self.process_imgs(imgs)
                sizes = [t.shape[-2:] for t in imgs]
            if samples is not None:
                d = self.pad_size_divisor
                shape = tuple(int(v) for v in batch.shape[-2:])
                for sample, hw in zip(samples, sizes):
                    _set_metainfo(sample, dict(batch_input_shape=shape, pad_shape=(round_up(hw[0], d), round_up(hw[1], d))))
            batch_inputs["imgs"] = batch
        return {"inputs": batch_inputs, "data_samples": samples}


def _set_metainfo(sample, info):
    if callable(getattr(sample, "set_metainfo", None)):
        sample.set_metainfo(info)
    elif isinstance(getattr(sample, "metainfo", None), dict):
        sample.metainfo.update(info)
    elif isinstance(sample, dict) and isinstance(sample.get("metainfo"), dict):
        sample["metainfo"].update(info)
