"""LoadPointsFromFile and LoadPointsFromMultiSweeps under the reference's names, keywords and result keys (M3D/datasets/
transforms/loading.py:554-695 and :316-453), the first two steps of the nuScenes configs' train_pipeline and test_pipeline.

LoadPointsFromFile reads `lidar_points.lidar_path` with np.fromfile into `points`, a float32 [n, len(use_dim)] array.

LoadPointsFromMultiSweeps sets the keyframe's column 4 to 0 and appends sweeps: with `lidar_sweeps`, all of them when there are
at most sweeps_num, the first sweeps_num in test_mode, else np.random.choice(len, sweeps_num, replace=False) -- the reference's
one generator call, in its place.  Each chosen sweep is read (`lidar_sweeps[i].lidar_points.lidar_path`), loses its rows with
|x| < 1 and |y| < 1 (remove_close), goes through `lidar_sweeps[i].lidar_points.lidar2sensor` in float64 and gets `timestamp -
lidar_sweeps[i].timestamp` in column 4.  Without `lidar_sweeps` and with pad_empty_sweeps the keyframe is appended sweeps_num
times more (through remove_close when set).  The rows' arithmetic is the sweep step of points_aug.PointsAugPlan, defined by
points_aug.torch_points_aug and equal to the reference's numpy expression bit for bit.

defer=False runs that step on the host.  defer=True leaves `points` as ONE contiguous float32 buffer [keyframe rows ; chosen
sweeps' raw rows] -- untouched file contents: the loader's worker does nothing but np.fromfile and one concatenate -- and writes
the step into data["points_aug_plan"], in front of ObjectSample's paste and the chain; Det3DDataPreprocessor.process_points runs
it on the device with the rest of the plan (csrc/points_aug.hip).  Deferral needs use_dim == range(load_dim), 5 <= load_dim <= 8.

LoadAnnotations3D (M3D/datasets/transforms/loading.py:832-1071), the step behind them, moves gt_bboxes_3d / gt_labels_3d /
attr_labels from `ann_info` to the root of the results; it touches no points.

BEVLoadMultiViewImageFromFiles (BF/loading.py:13-208, keywords of mmdet3d's LoadMultiViewImageFromFiles) is the first step of
the camera side.  From `images` (per camera img_path, cam2img, lidar2cam) it makes cam2img / lidar2cam / cam2lidar / lidar2img /
ori_cam2img with the reference's dtypes and operation order -- lidar2cam in float32, cam2lidar a float64 eye(4) filled from the
float32 transpose and -R^T t, cam2img a float32 eye(4) with the 3x3 block, lidar2img their float32 product -- and, with
num_ref_frames > 0, the reference's frame choice with its np.random.choice calls in its order (the files are then still
taken from `images`, as there).  The frames are JPEG files decoded by this package's own decoder (jpeg.py: bit for bit
Pillow's, which the reference calls): defer=False leaves `img` as the list of uint8 [H, W, 3] arrays (float32 with to_float32),
zero-padded to the largest; defer=True runs only the entropy stage in the worker and leaves a jpeg.JpegFrames -- headers and
coefficients, nothing decoded -- for Det3DDataPreprocessor to decode on the device.  A sample with a frame the fused decoder
does not take is decoded on the host with Pillow (one warning) and is the uint8 [N, H, W, 3] block instead.
"""
import copy
import warnings

import numpy as np
import torch

from . import jpeg
from . import points_aug as pa
from .registry import TRANSFORMS


def _use_dim(use_dim, load_dim):
    use_dim = list(range(use_dim)) if isinstance(use_dim, int) else [int(d) for d in use_dim]
    if max(use_dim) >= load_dim:
        raise ValueError("Expect all used dimensions < %d, got %s" % (load_dim, use_dim))
    return use_dim


def read_points(path, load_dim):
    """float32 [n, load_dim]: the file as it is."""
    return np.fromfile(path, dtype=np.float32).reshape(-1, load_dim)


@TRANSFORMS.register_module()
class LoadPointsFromFile:
    """points = the file's float32 [n, load_dim][:, use_dim].  The keywords this package has no use for are accepted at their
    defaults; backend_args is accepted and ignored (files are local)."""

    def __init__(self, coord_type, load_dim=6, use_dim=(0, 1, 2), shift_height=False, use_color=False, norm_intensity=False,
                 norm_elongation=False, backend_args=None):
        if coord_type not in ("CAMERA", "LIDAR", "DEPTH"):
            raise ValueError("coord_type must be 'CAMERA', 'LIDAR' or 'DEPTH', got %r" % (coord_type,))
        for name, value in (("shift_height", shift_height), ("use_color", use_color), ("norm_intensity", norm_intensity),
                            ("norm_elongation", norm_elongation)):
            if value:
                raise NotImplementedError("LoadPointsFromFile(%s=True) is not implemented" % name)
        self.coord_type, self.load_dim, self.use_dim = coord_type, int(load_dim), _use_dim(use_dim, int(load_dim))
        self.shift_height = self.use_color = self.norm_intensity = self.norm_elongation = False
        self.backend_args = backend_args

    def transform(self, data):
        points = read_points(data["lidar_points"]["lidar_path"], self.load_dim)
        data["points"] = points if self.use_dim == list(range(self.load_dim)) else points[:, self.use_dim]
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class LoadPointsFromMultiSweeps:
    """See the module docstring.  `points` (float32 [n, load_dim] array or tensor) comes back as the kind it came in."""

    def __init__(self, sweeps_num=10, load_dim=5, use_dim=(0, 1, 2, 4), backend_args=None, pad_empty_sweeps=False,
                 remove_close=False, test_mode=False, defer=False):
        self.load_dim, self.sweeps_num = int(load_dim), int(sweeps_num)
        self.use_dim = _use_dim(use_dim, self.load_dim)
        if self.load_dim < 5:
            raise ValueError("LoadPointsFromMultiSweeps writes the time lag into column 4: load_dim=%d" % self.load_dim)
        if defer and not (self.use_dim == list(range(self.load_dim)) and self.load_dim <= 8):
            raise ValueError("defer=True needs use_dim == range(load_dim) and 5 <= load_dim <= 8, got use_dim=%s, load_dim=%d; "
                             "use defer=False" % (self.use_dim, self.load_dim))
        self.backend_args = backend_args
        self.pad_empty_sweeps, self.remove_close, self.test_mode = bool(pad_empty_sweeps), bool(remove_close), bool(test_mode)
        self.defer = bool(defer)

    def _gather(self, data, key):
        """(the clouds [keyframe, sweep 1, ...] as read, lidar2sensor [S, 4, 4] or None, dt [S])."""
        if "lidar_sweeps" not in data:
            copies = self.sweeps_num if self.pad_empty_sweeps else 0
            return [key] * (1 + copies), None, np.zeros(copies, np.float32)
        sweeps = data["lidar_sweeps"]
        if len(sweeps) <= self.sweeps_num:
            choices = np.arange(len(sweeps))
        elif self.test_mode:
            choices = np.arange(self.sweeps_num)
        else:
            choices = np.random.choice(len(sweeps), self.sweeps_num, replace=False)
        ts = data["timestamp"]
        clouds, l2s, dt = [key], np.zeros((len(choices), 4, 4), np.float64), np.zeros(len(choices), np.float32)
        for i, idx in enumerate(choices):
            sweep = sweeps[idx]
            clouds.append(read_points(sweep["lidar_points"]["lidar_path"], self.load_dim))
            l2s[i] = np.array(sweep["lidar_points"]["lidar2sensor"])
            dt[i] = ts - sweep["timestamp"]  # a float64 difference stored as float32, as the reference's column assignment
        return clouds, l2s, dt

    def transform(self, data):
        points = data["points"]
        was_tensor = torch.is_tensor(points)
        key = points.numpy() if was_tensor else np.asarray(points)
        if key.dtype != np.float32 or key.ndim != 2 or key.shape[1] != self.load_dim:
            raise ValueError("points must be float32 [n, load_dim=%d], got %s %s" % (self.load_dim, key.dtype, key.shape))
        clouds, l2s, dt = self._gather(data, key)
        starts = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
        rows = np.concatenate(clouds, 0)
        if self.defer:
            pa._plan_of(data).set_sweeps(starts, l2s, dt, self.remove_close)
            data["points"] = torch.from_numpy(rows) if was_tensor else rows
            return data
        out = pa.torch_points_aug(rows, pa.PointsAugPlan().set_sweeps(starts, l2s, dt, self.remove_close))
        if self.use_dim != list(range(self.load_dim)):
            out = out[:, self.use_dim]
        data["points"] = out if was_tensor else out.numpy()
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class LoadAnnotations3D:
    """The reference's LoadAnnotations3D (M3D/datasets/transforms/loading.py:832-1071) for what the detection pipelines use of
    it: with_bbox_3d copies ann_info.gt_bboxes_3d to gt_bboxes_3d, with_label_3d ann_info.gt_labels_3d to gt_labels_3d,
    with_attr_label ann_info.attr_labels to attr_labels.  Boxes that come wrapped (anything with `.tensor`, as the reference's
    LiDARInstance3DBoxes) are handed on as their float32 tensor, arrays and tensors as they are: what the transforms behind
    it take (points_aug._unwrap).  Every other with_* flag raises NotImplementedError when set; poly2mask, seg_3d_dtype,
    seg_offset and dataset_type belong to those branches and are kept; backend_args is accepted and ignored."""
    _UNSUPPORTED = ("with_mask_3d", "with_seg_3d", "with_bbox", "with_label", "with_mask", "with_seg", "with_bbox_depth",
                    "with_panoptic_3d")

    def __init__(self, with_bbox_3d=True, with_label_3d=True, with_attr_label=False, with_mask_3d=False, with_seg_3d=False,
                 with_bbox=False, with_label=False, with_mask=False, with_seg=False, with_bbox_depth=False, with_panoptic_3d=False,
                 poly2mask=True, seg_3d_dtype="np.int64", seg_offset=None, dataset_type=None, backend_args=None):
        given = dict(with_mask_3d=with_mask_3d, with_seg_3d=with_seg_3d, with_bbox=with_bbox, with_label=with_label,
                     with_mask=with_mask, with_seg=with_seg, with_bbox_depth=with_bbox_depth, with_panoptic_3d=with_panoptic_3d)
        for name in self._UNSUPPORTED:
            if given[name]:
                raise NotImplementedError("LoadAnnotations3D(%s=True) is not implemented" % name)
            setattr(self, name, False)
        self.with_bbox_3d, self.with_label_3d, self.with_attr_label = bool(with_bbox_3d), bool(with_label_3d), bool(with_attr_label)
        self.poly2mask, self.seg_3d_dtype, self.seg_offset, self.dataset_type = poly2mask, seg_3d_dtype, seg_offset, dataset_type
        self.backend_args = backend_args

    def transform(self, results):
        ann = results["ann_info"]
        if self.with_bbox_3d:
            boxes = ann["gt_bboxes_3d"]
            results["gt_bboxes_3d"] = boxes.tensor if hasattr(boxes, "tensor") else boxes
        if self.with_label_3d:
            results["gt_labels_3d"] = ann["gt_labels_3d"]
        if self.with_attr_label:
            results["attr_labels"] = ann["attr_labels"]
        return results

    __call__ = transform


_warned_fallback = False


def _host_decode(stream, reason):
    """Pillow's decode of a stream the fused decoder does not take: uint8 [H, W, 3]."""
    global _warned_fallback
    if not _warned_fallback:
        _warned_fallback = True
        warnings.warn("BEVLoadMultiViewImageFromFiles: a frame is not taken by the fused JPEG decoder (%s); such samples are "
                      "decoded on the host with Pillow" % reason)
    import io
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("a frame needs the host JPEG decoder (%s) and Pillow is not installed" % reason) from e
    return np.asarray(Image.open(io.BytesIO(bytes(stream))).convert("RGB"))


def _pad_to(img, shape):
    """mmcv.impad(img, shape=shape, pad_val=0): zeros at the bottom and right."""
    if tuple(img.shape[:2]) == tuple(shape):
        return img
    out = np.zeros((shape[0], shape[1]) + img.shape[2:], dtype=img.dtype)
    out[:img.shape[0], :img.shape[1]] = img
    return out


@TRANSFORMS.register_module()
class BEVLoadMultiViewImageFromFiles:
    """See the module docstring.  color_type: 'unchanged' or 'color', on three-component files; backend_args is accepted and
    ignored (files are local)."""

    def __init__(self, to_float32=False, color_type="unchanged", backend_args=None, num_views=5, num_ref_frames=-1,
                 test_mode=False, set_default_scale=True, defer=False):
        if color_type not in ("unchanged", "color"):
            raise NotImplementedError("BEVLoadMultiViewImageFromFiles(color_type=%r) is not implemented" % (color_type,))
        self.to_float32, self.color_type, self.backend_args = bool(to_float32), color_type, backend_args
        self.num_views, self.num_ref_frames = num_views, num_ref_frames
        self.test_mode, self.set_default_scale = bool(test_mode), bool(set_default_scale)
        self.defer = bool(defer)
        if self.defer and self.to_float32:
            raise ValueError("defer=True leaves the frames undecoded: to_float32 has nothing to convert; use defer=False")

    def _choose_frames(self, results):
        """The num_ref_frames > 0 branch: picks the reference frames and re-bases their lidar2cam onto the current ego pose."""
        V, R = self.num_views, self.num_ref_frames
        num_frames = len(results["img_filename"]) // V - 1
        if num_frames == 0:  # no previous frame: the current one again
            choices = np.random.choice(1, R, replace=True)
        elif num_frames >= R:
            if self.test_mode:
                choices = np.arange(num_frames - R, num_frames) + 1
            else:
                choices = np.random.choice(num_frames, R, replace=False) + 1
        elif 0 < num_frames < R:
            if self.test_mode:
                choices = np.concatenate([np.arange(num_frames) + 1, np.random.choice(num_frames, R - num_frames, replace=True) + 1])
            else:
                choices = np.random.choice(num_frames, R, replace=True) + 1
        else:
            raise NotImplementedError
        choices = np.concatenate([np.array([0], dtype=np.int64), choices])
        pick = lambda seq: [item for c in choices for item in seq[c * V:(c + 1) * V]]  # noqa: E731
        results["img_filename"] = pick(results["img_filename"])
        for key in ("cam2img", "lidar2cam"):
            if key in results:
                results[key] = pick(results[key])
        if "ego2global" in results:
            results["ego2global"] = [results["ego2global"][c] for c in choices]
        if "lidar2cam" in results:
            def padded(m):
                out = np.eye(4)
                out[:m.shape[0], :m.shape[1]] = m
                return out
            for k in range(1, len(choices)):  # only the previous frames move
                cur2prev = np.linalg.inv(padded(results["ego2global"][k])).dot(padded(results["ego2global"][0]))
                for i in range(k * V, (k + 1) * V):
                    results["lidar2cam"][i] = results["lidar2cam"][i].dot(cur2prev)
        return choices

    def transform(self, results):
        if self.num_ref_frames > 0:
            self._choose_frames(results)
        filename, cam2img, lidar2cam, cam2lidar, lidar2img = [], [], [], [], []
        for cam in results["images"].values():
            filename.append(cam["img_path"])
            lidar2cam.append(cam["lidar2cam"])
            l2c = np.array(cam["lidar2cam"]).astype(np.float32)
            rot, trans = l2c[:3, :3], l2c[:3, 3:4]
            c2l = np.eye(4)
            c2l[:3, :3] = rot.T
            c2l[:3, 3:4] = -1 * np.matmul(rot.T, trans.reshape(3, 1))
            cam2lidar.append(c2l)
            c2i = np.eye(4).astype(np.float32)
            c2i[:3, :3] = np.array(cam["cam2img"]).astype(np.float32)
            cam2img.append(c2i)
            lidar2img.append(c2i @ l2c)
        results["img_path"] = filename
        results["cam2img"] = np.stack(cam2img, axis=0)
        results["lidar2cam"] = np.stack(lidar2cam, axis=0)
        results["cam2lidar"] = np.stack(cam2lidar, axis=0)
        results["lidar2img"] = np.stack(lidar2img, axis=0)
        results["ori_cam2img"] = copy.deepcopy(results["cam2img"])

        streams = [np.fromfile(name, dtype=np.uint8) for name in filename]
        headers = [jpeg.parse(s) for s in streams]
        unsupported = [h for h in headers if not h.supported]
        if unsupported:  # the whole sample on the host
            imgs = [_host_decode(s, jpeg.REASONS.get(unsupported[0].reason, "unsupported")) for s in streams]
            frames = None
        elif self.defer:
            frames = jpeg.JpegFrames.from_bytes(streams)
            imgs = None
        else:
            imgs = [jpeg.torch_jpeg_decode(*jpeg.entropy_decode(s, h)).numpy() for s, h in zip(streams, headers)]
            frames = None
        if imgs is not None:
            shapes = np.stack([img.shape for img in imgs], axis=0)
            assert shapes.min(0)[-1] == shapes.max(0)[-1]
            imgs = [_pad_to(img, tuple(shapes.max(0)[:2])) for img in imgs]
            shape = imgs[0].shape[:2]
            if self.defer:  # a sample the fused decoder does not take: the ordinary raw block
                results["img"] = np.stack(imgs, 0)
            else:
                results["img"] = [img.astype(np.float32) if self.to_float32 else img for img in imgs]
        else:
            shape = frames.shape[1:3]
            results["img"] = frames
        results["filename"] = filename
        results["img_shape"] = results["ori_shape"] = results["pad_shape"] = tuple(int(v) for v in shape)
        if self.set_default_scale:
            results["scale_factor"] = 1.0
        results["img_norm_cfg"] = dict(mean=np.zeros(3, dtype=np.float32), std=np.ones(3, dtype=np.float32), to_rgb=False)
        results["num_views"] = self.num_views
        results["num_ref_frames"] = self.num_ref_frames
        return results

    __call__ = transform
