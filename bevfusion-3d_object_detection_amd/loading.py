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
"""
import numpy as np
import torch

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
