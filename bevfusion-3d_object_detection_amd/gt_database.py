"""The ground-truth database ObjectSample / DataBaseSampler (object_sample.py) read: per annotated object one `.bin` file with the
points inside its box, relative to the box's bottom centre, and one info pickle {class name: [dict(name, path, image_idx, gt_idx,
box3d_lidar, num_points_in_gt, difficulty, group_id[, score])]}.  The serial builder of the reference under its own name
(tools/dataset_converters/create_gt_database.py:111-340), without its 2-D mask branch and without dataset classes:

    create_groundtruth_database(samples, pipeline, classes, data_path, info_prefix, used_classes=None, ...)

`samples`: a sequence of the reference's `data_info` dicts as Det3DDataset.get_data_info returns them (sample_idx, lidar_points,
lidar_sweeps, timestamp, ann_info with gt_bboxes_3d / gt_labels_3d and optionally group_ids / difficulty / score), or an object
with __len__ and get_data_info.  `pipeline`: transform dicts (built through registry.TRANSFORMS) or built transforms;
`nuscenes_pipeline()` is the reference's three steps for NuScenesDataset.  `classes`: the label -> name list (metainfo.classes).

Per sample the points go to the device once -- with a deferred pipeline (`points_aug_plan` in the sample) the sweep merge runs
there through points_aug.process_points and the operator reads its result in place -- then box_ops.points_in_boxes with
center=True: one small upload (planes and centres), three launches, and two reads, the counts and the gathered rows.  The files
are slices of that one host array.  device="cpu" (or None without a GPU) runs the torch specification; the bytes are the same.
"""
import os
import pickle

import numpy as np
import torch

from . import box_ops
from . import points_aug as pa
from .registry import TRANSFORMS


def nuscenes_pipeline(defer=False):
    """The reference's pipeline for NuScenesDataset (create_gt_database.py:177-193).  defer: the sweep merge runs on the device."""
    return [dict(type="LoadPointsFromFile", coord_type="LIDAR", load_dim=5, use_dim=5),
            dict(type="LoadPointsFromMultiSweeps", sweeps_num=10, use_dim=[0, 1, 2, 3, 4], pad_empty_sweeps=True, remove_close=True,
                 defer=bool(defer)),
            dict(type="LoadAnnotations3D", with_bbox_3d=True, with_label_3d=True)]


def _to_numpy(value):
    value = getattr(value, "tensor", value)
    return value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)


def _device(device):
    if device is None:
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    return torch.device(device)


def sample_points(example, dev):
    """float32 [n, C] tensor on `dev`: the sample's points, the deferred steps of its plan applied."""
    points = getattr(example["points"], "tensor", example["points"])
    points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)) if isinstance(points, np.ndarray) else points
    points = points.to(device=dev, dtype=torch.float32)  # the sample's one upload
    plan = example.get("points_aug_plan")
    return points if plan is None else pa.process_points([points], [plan])[0]


def object_points(example, dev):
    """(counts int32 array [K], rows float32 array [sum(counts), C]) of one loaded sample: per box of ann_info.gt_bboxes_3d its
    member rows, centred (box_ops.points_in_boxes); two host reads."""
    boxes = np.ascontiguousarray(_to_numpy(example["ann_info"]["gt_bboxes_3d"]), dtype=np.float32)
    counts, rows = box_ops.points_in_boxes(sample_points(example, dev), boxes, center=True)
    return counts.numpy(), rows.cpu().numpy()


def create_groundtruth_database(samples, pipeline, classes, data_path, info_prefix, used_classes=None, database_save_path=None,
                                db_info_save_path=None, relative_path=True, with_mask=False, device=None):
    """Writes `database_save_path`/{sample_idx}_{name}_{i}.bin for EVERY object and the info pickle `db_info_save_path` with the
    objects whose class is in `used_classes` (None: all); returns the infos.  See the module docstring."""
    if with_mask:
        raise NotImplementedError("create_groundtruth_database(with_mask=True): the 2-D mask branch (pycocotools, mmcv) is not "
                                  "implemented")
    dev = _device(device)
    steps = [TRANSFORMS.build(step) if isinstance(step, dict) else step for step in pipeline]
    if database_save_path is None:
        database_save_path = os.path.join(data_path, "%s_gt_database" % info_prefix)
    if db_info_save_path is None:
        db_info_save_path = os.path.join(data_path, "%s_dbinfos_train.pkl" % info_prefix)
    os.makedirs(database_save_path, exist_ok=True)
    all_db_infos = dict()
    group_counter = 0
    for j in range(len(samples)):
        example = samples.get_data_info(j) if hasattr(samples, "get_data_info") else dict(samples[j])
        for step in steps:
            example = step(example)
        annos = example["ann_info"]
        image_idx = example["sample_idx"]
        gt_boxes_3d = _to_numpy(annos["gt_bboxes_3d"])
        names = [classes[int(i)] for i in annos["gt_labels_3d"]]
        num_obj = gt_boxes_3d.shape[0]
        group_dict = dict()
        group_ids = annos["group_ids"] if "group_ids" in annos else np.arange(num_obj, dtype=np.int64)
        difficulty = annos["difficulty"] if "difficulty" in annos else np.zeros(num_obj, dtype=np.int32)
        counts, rows = object_points(example, dev)
        starts = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        for i in range(num_obj):
            filename = "%s_%s_%d.bin" % (image_idx, names[i], i)
            abs_filepath = os.path.join(database_save_path, filename)
            rel_filepath = os.path.join("%s_gt_database" % info_prefix, filename)
            gt_points = rows[starts[i]:starts[i + 1]]
            gt_points.tofile(abs_filepath)
            if used_classes is None or names[i] in used_classes:
                db_info = {"name": names[i], "path": rel_filepath if relative_path else abs_filepath, "image_idx": image_idx,
                           "gt_idx": i, "box3d_lidar": gt_boxes_3d[i], "num_points_in_gt": gt_points.shape[0],
                           "difficulty": difficulty[i]}
                local_group_id = group_ids[i]
                if local_group_id not in group_dict:
                    group_dict[local_group_id] = group_counter
                    group_counter += 1
                db_info["group_id"] = group_dict[local_group_id]
                if "score" in annos:
                    db_info["score"] = annos["score"][i]
                all_db_infos.setdefault(names[i], []).append(db_info)
    with open(db_info_save_path, "wb") as f:
        pickle.dump(all_db_infos, f)
    return all_db_infos
