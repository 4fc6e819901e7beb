"""CPU: LoadAnnotations3D under the reference's name, keywords and defaults, and the three-step pipeline of the reference's
database builder built by name."""
import inspect

import numpy as np
import pytest
import torch

from bevfusion_amd import gt_database
from bevfusion_amd.loading import LoadAnnotations3D
from bevfusion_amd.registry import TRANSFORMS


def _ann():
    return dict(gt_bboxes_3d=np.arange(14, dtype=np.float32).reshape(2, 7), gt_labels_3d=np.array([1, 0], np.int64),
                attr_labels=np.array([3, 4], np.int64))


def test_keywords_and_defaults_are_the_reference_s():
    params = inspect.signature(LoadAnnotations3D.__init__).parameters
    want = dict(with_bbox_3d=True, with_label_3d=True, with_attr_label=False, with_mask_3d=False, with_seg_3d=False, with_bbox=False,
                with_label=False, with_mask=False, with_seg=False, with_bbox_depth=False, with_panoptic_3d=False, poly2mask=True,
                seg_3d_dtype="np.int64", seg_offset=None, dataset_type=None, backend_args=None)
    assert [p for p in params if p != "self"] == list(want)
    assert {k: params[k].default for k in want} == want


def test_default_moves_boxes_and_labels():
    data = dict(ann_info=_ann(), points=np.zeros((3, 5), np.float32))
    out = LoadAnnotations3D()(data)
    assert out is data and out["gt_bboxes_3d"] is data["ann_info"]["gt_bboxes_3d"] and out["gt_labels_3d"] is data["ann_info"]["gt_labels_3d"]
    assert "attr_labels" not in out and "ann_info" in out
    out = LoadAnnotations3D(with_bbox_3d=False, with_label_3d=False, with_attr_label=True, backend_args=dict(backend="disk")).transform(
        dict(ann_info=_ann()))
    assert sorted(out) == ["ann_info", "attr_labels"] and out["attr_labels"].tolist() == [3, 4]


def test_boxes_as_tensor_or_wrapped():
    t = torch.arange(18, dtype=torch.float32).reshape(2, 9)
    out = LoadAnnotations3D()(dict(ann_info=dict(_ann(), gt_bboxes_3d=t)))
    assert out["gt_bboxes_3d"] is t

    class Boxes:
        tensor = t

    out = LoadAnnotations3D()(dict(ann_info=dict(_ann(), gt_bboxes_3d=Boxes())))
    assert out["gt_bboxes_3d"] is t
    # what the transforms behind it take
    ranged = TRANSFORMS.build(dict(type="ObjectRangeFilter", point_cloud_range=[-54, -54, -5, 54, 54, 3]))(out)
    assert torch.is_tensor(ranged["gt_bboxes_3d"]) and ranged["gt_bboxes_3d"].shape == (2, 9)


@pytest.mark.parametrize("flag", ["with_mask_3d", "with_seg_3d", "with_bbox", "with_label", "with_mask", "with_seg", "with_bbox_depth",
                                  "with_panoptic_3d"])
def test_unsupported_flags_raise(flag):
    with pytest.raises(NotImplementedError, match=flag):
        LoadAnnotations3D(**{flag: True})


def test_builds_by_name():
    assert "LoadAnnotations3D" in TRANSFORMS
    step = TRANSFORMS.build(dict(type="LoadAnnotations3D", with_bbox_3d=True, with_label_3d=True))
    assert isinstance(step, LoadAnnotations3D) and step.with_bbox_3d and step.with_label_3d and not step.with_attr_label


@pytest.mark.parametrize("defer", [False, True])
def test_nuscenes_pipeline_builds_by_name(defer):
    cfg = gt_database.nuscenes_pipeline(defer=defer)
    assert [c["type"] for c in cfg] == ["LoadPointsFromFile", "LoadPointsFromMultiSweeps", "LoadAnnotations3D"]
    steps = [TRANSFORMS.build(c) for c in cfg]
    assert steps[0].load_dim == 5 and steps[0].use_dim == [0, 1, 2, 3, 4]
    assert steps[1].sweeps_num == 10 and steps[1].use_dim == [0, 1, 2, 3, 4] and steps[1].pad_empty_sweeps and steps[1].remove_close
    assert steps[1].defer is defer and not steps[1].test_mode
    assert steps[2].with_bbox_3d and steps[2].with_label_3d
    assert [c["type"] for c in gt_database.nuscenes_pipeline()] == [c["type"] for c in cfg]
