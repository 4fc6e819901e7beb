"""ObjectSample (GT-paste) and its DataBaseSampler under the reference's names and keywords (M3D/datasets/transforms/
transforms_3d.py:328-460, dbsampler.py), the transform in front of GlobalRotScaleTrans in the LiDAR configs.

Host work, as in the reference and with its np.random calls in its order (one np.random.shuffle per class at construction, in
the info file's key order; a reshuffle when a class's index wraps): choosing the objects, the bird's-eye-view collision test,
reading the objects' .bin files, translating their points to their boxes (float32), the boxes and labels.  The info file is a
pickle {class name: [dict(name, path, box3d_lidar, num_points_in_gt, difficulty, ...)]}.

The points' part -- drop the original points inside any pasted box, put the pasted points in front -- is the paste step of
points_aug.PointsAugPlan, defined by points_aug.torch_points_aug: defer=False runs it on the host; defer=True writes it into
data["points_aug_plan"], leaves data["points"] untouched, and Det3DDataPreprocessor.process_points runs it on the device with
the rest of the plan (csrc/points_aug.hip).

`box_collision_test` restates data_augment_utils.box_collision_test as compiled numba executes it, vectorised over the pairs:
for two boxes whose axis-aligned hulls overlap, an edge of one crossing an edge of the other, or either box holding all four
corners of the other."""
import copy
import os
import pickle

import numpy as np
import torch

from . import points_aug as pa
from .registry import TRANSFORMS


def box_collision_test(boxes, qboxes, clockwise=True):
    """boxes [N, 4, 2], qboxes [K, 4, 2] corners (points_aug.box_corners) -> bool [N, K], in the corners' arithmetic."""
    nxt = [1, 2, 3, 0]
    lo = np.maximum(boxes.min(1)[:, None, :], qboxes.min(1)[None, :, :])
    hi = np.minimum(boxes.max(1)[:, None, :], qboxes.max(1)[None, :, :])
    near = ((hi - lo) > 0).all(-1)                                         # [N, K]: the standup boxes overlap
    A, B = boxes[:, None, :, None, :], boxes[:, nxt][:, None, :, None, :]  # edge k of box i
    C, D = qboxes[None, :, None, :, :], qboxes[:, nxt][None, :, None, :, :]  # edge l of qbox j

    def ccw(p, q, r):  # the reference's acd / bcd / abc / abd
        return (r[..., 1] - p[..., 1]) * (q[..., 0] - p[..., 0]) > (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0])

    cross = ((ccw(A, C, D) != ccw(B, C, D)) & (ccw(A, B, C) != ccw(A, B, D))).any((2, 3))

    def holds(outer, inner):  # [len(outer), len(inner)]: every corner of `inner` strictly inside `outer`
        vec = outer - outer[:, nxt]
        if clockwise:
            vec = -vec
        diff = outer[:, None, None, :, :] - inner[None, :, :, None, :]     # [outer, inner, corner l, edge k, xy]
        c = vec[:, None, None, :, 1] * diff[..., 0]
        c = c - vec[:, None, None, :, 0] * diff[..., 1]
        return (c < 0).all((2, 3))

    return near & (cross | holds(boxes, qboxes) | holds(qboxes, boxes).T)


class BatchSampler:
    """Walks a shuffled index of one class's objects; reshuffles when it reaches the end."""

    def __init__(self, sampled_list, name=None, epoch=None, shuffle=True, drop_reminder=False):
        self._sampled_list = sampled_list
        self._indices = np.arange(len(sampled_list))
        if shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0
        self._example_num = len(sampled_list)
        self._name, self._shuffle, self._epoch, self._drop_reminder = name, shuffle, epoch, drop_reminder

    def _sample(self, num):
        if self._idx + num >= self._example_num:  # the rest, however few, then a new order
            ret = self._indices[self._idx:].copy()
            self._reset()
        else:
            ret = self._indices[self._idx:self._idx + num]
            self._idx += num
        return ret

    def _reset(self):
        assert self._name is not None
        if self._shuffle:
            np.random.shuffle(self._indices)
        self._idx = 0

    def sample(self, num):
        return [self._sampled_list[i] for i in self._sample(num)]


@TRANSFORMS.register_module()
class DataBaseSampler:
    """The ground-truth database: per class a BatchSampler over the objects `prepare` leaves.  points_loader: load_dim floats
    per point in the objects' .bin files, use_dim the columns kept (an int n: the first n)."""

    def __init__(self, info_path, data_root, rate, prepare, sample_groups, classes=None,
                 points_loader=dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=4, use_dim=[0, 1, 2, 3]),
                 backend_args=None):
        self.data_root, self.info_path, self.rate, self.prepare, self.classes = data_root, info_path, rate, prepare, classes
        self.cat2label = {name: i for i, name in enumerate(classes)}
        self.label2cat = {i: name for i, name in enumerate(classes)}
        self.load_dim = int(points_loader.get("load_dim", 6))
        use_dim = points_loader.get("use_dim", [0, 1, 2])
        self.use_dim = list(range(use_dim)) if isinstance(use_dim, int) else list(use_dim)
        if max(self.use_dim) >= self.load_dim:
            raise ValueError("points_loader: use_dim %s needs more than load_dim=%d columns" % (self.use_dim, self.load_dim))
        with open(info_path, "rb") as f:
            db_infos = pickle.load(f)
        for prep_func, val in prepare.items():
            db_infos = getattr(self, prep_func)(db_infos, val)
        self.db_infos = self.group_db_infos = db_infos
        self.sample_groups = [{name: int(num)} for name, num in sample_groups.items()]
        self.sample_classes = [name for name in sample_groups]
        self.sample_max_nums = [int(num) for num in sample_groups.values()]
        self.sampler_dict = {k: BatchSampler(v, k, shuffle=True) for k, v in db_infos.items()}

    @staticmethod
    def filter_by_difficulty(db_infos, removed_difficulty):
        return {key: [info for info in infos if info["difficulty"] not in removed_difficulty] for key, infos in db_infos.items()}

    @staticmethod
    def filter_by_min_points(db_infos, min_gt_points_dict):
        for name, min_num in min_gt_points_dict.items():
            if int(min_num) > 0:
                db_infos[name] = [info for info in db_infos[name] if info["num_points_in_gt"] >= int(min_num)]
        return db_infos

    def load_points(self, info):
        """float32 tensor [n, len(use_dim)]: the object's points, relative to its box centre."""
        path = os.path.join(self.data_root, info["path"]) if self.data_root else info["path"]
        return torch.from_numpy(np.fromfile(path, dtype=np.float32).reshape(-1, self.load_dim)[:, self.use_dim])

    def sample_all(self, gt_bboxes, gt_labels, img=None, ground_plane=None):
        """gt_bboxes [M, 7+] array, gt_labels [M] -> None, or dict(gt_labels_3d int [K], gt_bboxes_3d [K, 7+], points float32
        tensor [m, C] in sampling order, group_ids).  Per class of sample_groups, round(rate * (its number - how many the
        frame holds)) objects are drawn and those that collide with a box already there, or pasted before, are dropped."""
        nums = []
        for name, max_num in zip(self.sample_classes, self.sample_max_nums):
            label = self.cat2label[name]
            num = int(max_num - np.sum([n == label for n in gt_labels]))
            nums.append(np.round(self.rate * num).astype(np.int64))
        sampled, sampled_boxes, avoid = [], [], gt_bboxes
        for name, num in zip(self.sample_classes, nums):
            if num > 0:
                chosen = self.sample_class_v2(name, num, avoid)
                sampled += chosen
                if chosen:
                    box = np.stack([s["box3d_lidar"] for s in chosen], axis=0)
                    sampled_boxes.append(box)
                    avoid = np.concatenate([avoid, box], axis=0)
        if not sampled:
            return None
        sampled_boxes = np.concatenate(sampled_boxes, axis=0)
        points = []
        for info in sampled:
            p = self.load_points(info)
            p[:, :3] += p.new_tensor(info["box3d_lidar"][:3])
            points.append(p)
        labels = np.array([self.cat2label[s["name"]] for s in sampled], dtype=int)
        if ground_plane is not None:
            dz = (ground_plane[:3][None, :] * sampled_boxes[:, :3]).sum(-1) + ground_plane[3]
            sampled_boxes[:, 2] -= dz
            for p, d in zip(points, dz):
                p[:, 2].sub_(d)
        return dict(gt_labels_3d=labels, gt_bboxes_3d=sampled_boxes, points=torch.cat(points, 0),
                    group_ids=np.arange(gt_bboxes.shape[0], gt_bboxes.shape[0] + len(sampled)))

    def sample_class_v2(self, name, num, gt_bboxes):
        """`num` objects of class `name` from its sampler, less those that collide in the bird's-eye view with gt_bboxes or
        with an earlier one of the same draw."""
        sampled = copy.deepcopy(self.sampler_dict[name].sample(num))
        num_gt = gt_bboxes.shape[0]
        sp_boxes = np.stack([s["box3d_lidar"] for s in sampled], axis=0)
        sp_boxes = np.concatenate([gt_bboxes, sp_boxes], axis=0)[num_gt:]  # in the dtype the two have in common
        total_bv = np.concatenate([pa.box_corners(gt_bboxes[:, 0:2], gt_bboxes[:, 3:5], gt_bboxes[:, 6], 0.5),
                                   pa.box_corners(sp_boxes[:, 0:2], sp_boxes[:, 3:5], sp_boxes[:, 6], 0.5)], axis=0)
        coll = box_collision_test(total_bv, total_bv)
        diag = np.arange(total_bv.shape[0])
        coll[diag, diag] = False
        valid = []
        for i in range(num_gt, num_gt + len(sampled)):
            if coll[i].any():
                coll[i] = False
                coll[:, i] = False
            else:
                valid.append(sampled[i - num_gt])
        return valid


@TRANSFORMS.register_module()
class ObjectSample:
    """Pastes objects of the database into the frame: their boxes and labels (int64) are appended to gt_bboxes_3d /
    gt_labels_3d, the frame's points inside a pasted box are dropped and the objects' points go in front of the rest.
    `disabled` (what the reference's DisableObjectSampleHook sets): the transform does nothing, draws nothing."""

    def __init__(self, db_sampler, sample_2d=False, use_ground_plane=False, defer=False):
        if sample_2d:
            raise NotImplementedError("ObjectSample(sample_2d=True): image patches are not pasted (the reference's "
                                      "DataBaseSampler.sample_all does not take the 2-D arguments either)")
        self.sampler_cfg = db_sampler
        self.sample_2d = False
        if isinstance(db_sampler, dict):
            db_sampler = TRANSFORMS.build(dict(db_sampler, type=db_sampler.get("type", "DataBaseSampler")))
        self.db_sampler = db_sampler
        self.use_ground_plane, self.defer = bool(use_ground_plane), bool(defer)
        self.disabled = False

    def transform(self, data):
        if self.disabled:
            return data
        boxes, labels = data["gt_bboxes_3d"], data["gt_labels_3d"]
        ground_plane = None
        if self.use_ground_plane:
            ground_plane = data.get("plane")
            if ground_plane is None:
                raise ValueError("`use_ground_plane` is True but data['plane'] is None")
        boxes_np = boxes.numpy() if torch.is_tensor(boxes) else np.asarray(boxes)
        labels_np = labels.numpy() if torch.is_tensor(labels) else np.asarray(labels)
        sampled = self.db_sampler.sample_all(boxes_np, labels_np, img=None, ground_plane=ground_plane)
        if sampled is not None:
            labels_np = np.concatenate([labels_np, sampled["gt_labels_3d"]], axis=0)
            boxes_np = np.concatenate([boxes_np, sampled["gt_bboxes_3d"]]).astype(boxes_np.dtype)
            if self.defer:
                pa._plan_of(data).set_paste(sampled["points"].numpy(), sampled["gt_bboxes_3d"])
            else:
                pa._apply(data, pa.PointsAugPlan().set_paste(sampled["points"].numpy(), sampled["gt_bboxes_3d"]))
        labels_np = labels_np.astype(np.int64)
        data["gt_bboxes_3d"] = torch.from_numpy(boxes_np) if torch.is_tensor(boxes) else boxes_np
        data["gt_labels_3d"] = torch.from_numpy(labels_np) if torch.is_tensor(labels) else labels_np
        return data

    __call__ = transform
