"""CPU: the reference's own `custom_data` configuration (projects/BEVFusion/configs/custom_data/) as a model dict of this
package -- compared key by key with the reference's merged `model` dict (tests/golden/custom_data_model_cfg.json, written
by tests/golden/make_custom_cfg_golden.py), built on the CPU, and the synthetic inputs of its shapes."""
import hashlib
import json
import os
import re

import numpy as np

import bevfusion_amd  # noqa: F401
from bevfusion_amd import synthetic
from bevfusion_amd.bevfusion import CONFIGS, custom_data_config, model_config, nuscenes_config
from bevfusion_amd.registry import MODELS

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "custom_data_model_cfg.json")

# reference keys this package leaves out on purpose (regular expressions over the dotted path)
OMITTED = [
    r".*\.(norm_cfg|act_cfg|conv_cfg)(\..*)?",      # our modules fix the layer kinds (SECOND / SECONDFPN / LSS-FPN / FFN / LN) ...
    r"pts_neck\.upsample_cfg(\..*)?",               # ... and the SECONDFPN's deconv
    r"img_backbone\.init_cfg(\..*)?",               # a checkpoint on the fork author's disk
    r"data_preprocessor\.(mean|std)",               # image normalisation belongs to the data pipeline
    r"data_preprocessor\.type",                     # layer type names our registry does not use
    r"bbox_head\.decoder_layer\.type",
]
# ... except the norm_cfg dicts our SECOND / SECONDFPN / sparse encoder do read (eps, momentum): those we carry
CARRIED_NORM = ("pts_backbone.norm_cfg", "pts_neck.norm_cfg", "pts_middle_encoder.norm_cfg")


def _norm(v):
    if isinstance(v, dict):
        return {k: _norm(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_norm(x) for x in v]
    return v


def _leaves(d, prefix=""):
    for k, v in d.items():
        path = prefix + k
        if isinstance(v, dict):
            yield from _leaves(v, path + ".")
        else:
            yield path, v


def test_custom_config_matches_the_reference_fixture():
    with open(GOLDEN) as f:
        ref = json.load(f)
    ours = _norm(custom_data_config())
    ours_leaves, ref_leaves = dict(_leaves(ours)), dict(_leaves(ref))
    for path, v in ours_leaves.items():      # every key we carry is the reference's, with the reference's value
        assert path in ref_leaves, "not in the reference: " + path
        assert v == ref_leaves[path], (path, v, ref_leaves[path])
    for path in ref_leaves:                   # every reference key we lack is left out on purpose
        if path not in ours_leaves:
            assert any(re.fullmatch(pat, path) for pat in OMITTED), "missing without a reason: " + path
    for path in CARRIED_NORM:
        assert path + ".eps" in ours_leaves
    # the values the custom setup is about
    assert ours["bbox_head"]["num_proposals"] == 500 and ours["bbox_head"]["num_classes"] == 5
    assert ours["bbox_head"]["train_cfg"]["code_weights"] == [1.0] * 8 + [0.0, 0.0]
    assert ours["pts_middle_encoder"]["in_channels"] == 3 and ours["pts_voxel_encoder"]["num_features"] == 3
    assert ours["view_transform"]["image_size"] == [384, 704] and ours["view_transform"]["feature_size"] == [48, 88]
    assert ours["img_backbone"]["type"] == "mmdet.SwinTransformer" and ours["img_neck"]["in_channels"] == [192, 384, 768]


def test_custom_config_variants_and_names():
    assert CONFIGS["custom_data"] is custom_data_config and CONFIGS["nuscenes"] is nuscenes_config
    assert model_config("custom_data", camera=False) == custom_data_config(camera=False)
    lidar = custom_data_config(camera=False)
    assert "img_backbone" not in lidar and "view_transform" not in lidar and "fusion_layer" not in lidar
    assert lidar["pts_backbone"]["in_channels"] == 256
    with open(GOLDEN) as f:
        ref = json.load(f)
    ref_leaves = dict(_leaves(ref))
    for path, v in _leaves(_norm(lidar)):   # the LiDAR-only dict is a subset of the merged one as well
        assert ref_leaves[path] == v, path
    # building the custom dict leaves the nuScenes one as it was
    assert nuscenes_config()["bbox_head"]["num_proposals"] == 200 and nuscenes_config()["bbox_head"]["num_classes"] == 10


def test_custom_model_builds_on_the_cpu():
    model = MODELS.build(custom_data_config())
    w = model.pts_middle_encoder.conv_input[0].weight       # [Cout, kz, ky, kx, Cin]
    assert w.shape[0] == 16 and w.shape[-1] == 3
    head = model.bbox_head
    assert head.num_proposals == 500 and head.num_classes == 5
    assert head.heatmap_head[-1].weight.shape[0] == 5
    assert head.class_encoding.in_channels == 5
    assert head.prediction_heads[0].heads["heatmap"][0] == 5
    assert tuple(model.view_transform.frustum.shape[:3]) == (118, 48, 88)
    assert head.train_cfg["code_weights"][-2:] == [0.0, 0.0]
    assert model.img_neck.in_channels == [192, 384, 768]


def _checksum(d):
    h = hashlib.sha256()
    for k in sorted(d):
        h.update(k.encode())
        h.update(np.ascontiguousarray(d[k]).tobytes())
    return h.hexdigest()


def test_synthetic_custom_shapes_and_unchanged_defaults():
    rig = synthetic.camera_rig(batch=2, **synthetic.CUSTOM["rig"])
    for k in ("camera_intrinsics", "camera2lidar", "lidar2image", "img_aug_matrix"):
        assert rig[k].shape == (2, 5, 4, 4) and rig[k].dtype == np.float32, k
    assert rig["lidar_aug_matrix"].shape == (2, 4, 4)
    aug = rig["img_aug_matrix"][0, 0]
    assert np.allclose(aug[[0, 1], [0, 1]], 0.48) and aug[0, 3] == -32.0 and aug[1, 3] == -48.0
    # the first five cameras of the nominal rig
    full = synthetic.camera_rig(batch=2)
    assert np.array_equal(rig["camera2lidar"], full["camera2lidar"][:, :5])
    assert np.array_equal(rig["lidar2image"], full["lidar2image"][:, :5])
    # the 704 x 384 window lies inside the resized 1600 x 900 source
    assert 32 + 704 <= 0.48 * 1600 and 48 + 384 <= 0.48 * 900
    # default arguments: byte-identical to the arrays before the options existed (sha256 taken on the parent commit)
    assert _checksum(synthetic.camera_rig()) == "532d63e8568352ce82d47636d02f9f5199111608cfeac8f2301b63ef7fa814d1"
    assert (_checksum(synthetic.camera_rig(batch=2, seed=1, train_aug=True))
            == "c817cbe2eb69ea5a73d101466c2255b76f42b490dcd6dc210b7fa246c6ed88a0")
    b, l = synthetic.gt_boxes()
    assert _checksum(dict(b=b, l=l)) == "8ecb8a56fb0bd819bab1bc686ac91a93ce46343686a7eefcdbb9b284f25b71cd"
    # custom classes: labels 0..4, sizes drawn from the five rows
    seen = set()
    for seed in range(3000, 3006):
        boxes, labels = synthetic.gt_boxes(seed=seed, classes=synthetic.CUSTOM["classes"])
        assert boxes.shape == (len(labels), 9) and labels.dtype == np.int64 and labels.min() >= 0 and labels.max() < 5
        rows = np.asarray(synthetic.CUSTOM["classes"])[labels]
        ratio = boxes[:, 3:6] / synthetic._CLASS_SIZES[rows]
        assert (ratio > 0.84).all() and (ratio < 1.21).all()
        seen |= set(labels.tolist())
    assert seen == {0, 1, 2, 3, 4}
    assert synthetic.lidar_sweep(1000, features=3).shape == (1000, 3)
