"""GPU: the reference's own `custom_data` model (bevfusion.custom_data_config: five 384 x 704 cameras, three point features,
five classes, 500 proposals, Swin-T) runs forward + backward through the HIP operators, its decoder's cross attention on
the split-key kernels; the real loss against oracle/head_oracle.py at these sizes.  Follows tests/test_model_gpu.py."""
import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import attention, synthetic
from bevfusion_amd.bevfusion import custom_data_config, surrogate_loss
from bevfusion_amd.registry import MODELS

pytestmark = pytest.mark.gpu
C = synthetic.CUSTOM


def _inputs(dev, B, camera=True):
    d = {"points": [torch.from_numpy(synthetic.lidar_sweep(40000, seed=1000 + i, features=C["point_features"])).to(dev)
                    for i in range(B)]}
    if camera:
        rig = synthetic.camera_rig(batch=B, seed=1, train_aug=True, **C["rig"])
        d["imgs"] = torch.randn(B, C["num_cams"], 3, *C["image_size"], device=dev)
        for src, dst in (("lidar2image", "lidar2img"), ("camera_intrinsics", "cam2img"), ("camera2lidar", "cam2lidar"),
                         ("img_aug_matrix", "img_aug_matrix"), ("lidar_aug_matrix", "lidar_aug_matrix")):
            d[dst] = torch.from_numpy(rig[src]).to(dev)
    return d


def _gts(B):
    return [tuple(torch.from_numpy(a) for a in synthetic.gt_boxes(seed=3000 + i, classes=C["classes"])) for i in range(B)]


def test_custom_full_model_forward_backward_bf16(dev, monkeypatch):
    """Camera + LiDAR + fusion + head at B = 1 under bf16 autocast; the 500-query cross attention takes the kernel."""
    torch.manual_seed(0)
    model = MODELS.build(custom_data_config()).to(dev).train()
    calls = []
    real = attention.cross_attention
    monkeypatch.setattr(attention, "cross_attention", lambda *a, **kw: (calls.append(tuple(a[0].shape)), real(*a, **kw))[1])
    inp = _inputs(dev, 1)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feats, depth_loss = model.extract_feat(inp)
        assert feats[0].shape == (1, 512, 180, 180)
        outs = model.bbox_head(feats)
        res = outs[0][0]
        assert res["heatmap"].shape == (1, 5, 500) and res["center"].shape == (1, 2, 500)
        assert res["dense_heatmap"].shape == (1, 5, 180, 180)
        loss = surrogate_loss(outs, depth_loss)
    assert calls == [(1, 500, 128)]  # one decoder layer, one cross attention, on csrc/attn.hip
    assert torch.isfinite(loss)
    loss.backward()
    for name in ("img_backbone", "img_neck", "view_transform", "pts_middle_encoder", "fusion_layer", "pts_backbone", "pts_neck",
                 "bbox_head"):
        grads = [p.grad for p in getattr(model, name).parameters() if p.requires_grad]
        assert all(g is not None and torch.isfinite(g).all() for g in grads), name
    assert model.view_transform.depthnet[0].weight.grad.abs().sum() > 0
    assert model.pts_middle_encoder.conv_input[0].weight.grad.abs().sum() > 0
    assert model.bbox_head.decoder[0].cross_attn.attn.in_proj_weight.grad.abs().sum() > 0


def test_custom_lidar_only_forward_backward_fp32(dev):
    """LiDAR-only, B = 2, fp32: three point features through the sparse encoder (odd Cin), 500 proposals."""
    torch.manual_seed(0)
    model = MODELS.build(custom_data_config(camera=False)).to(dev).train()
    outs, _ = model(_inputs(dev, 2, camera=False))
    res = outs[0][0]
    assert res["dense_heatmap"].shape == (2, 5, 180, 180)
    assert res["center"].shape == (2, 2, 500) and res["heatmap"].shape == (2, 5, 500)
    surrogate_loss(outs).backward()
    enc = model.pts_middle_encoder
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters() if p.requires_grad)
    assert enc.conv_input[0].weight.shape[-1] == 3 and enc.conv_input[0].weight.grad.abs().sum() > 0


def _check_losses_against_oracle(model, preds, gts, losses, dev, rel=1e-4):
    """tests/test_model_gpu.py::_check_losses_against_oracle with the class count and proposal count of the model instead
    of the nuScenes constants (oracle/head_oracle.py takes its sizes from its inputs)."""
    from bevfusion_amd import head_targets as ht
    from oracle import head_oracle as ho
    head = model.bbox_head
    res = {k: v.detach().float().cpu().numpy() for k, v in preds[0][0].items() if torch.is_tensor(v)}
    tc = head.train_cfg
    cfg = dict(point_cloud_range=tc["point_cloud_range"], voxel_size=tc["voxel_size"], out_size_factor=8,
               grid_size=tc["grid_size"], num_classes=head.num_classes, code_size=10, gaussian_overlap=0.1, min_radius=2,
               pos_weight=-1, assigner=dict(cls_w=0.15, alpha=0.25, gamma=2.0, reg_w=0.25, iou_w=0.25))
    gt_boxes, gt_labels, n_gt, _ = ht.pack_gt(gts, dev)
    p0 = preds[0][0]
    boxes_dev = head.bbox_coder.decode_boxes(p0["rot"], p0["dim"], p0["center"], p0["height"], p0["vel"])
    assert boxes_dev.shape[1] == head.num_proposals
    assigned_dev, _, cost_dev, _ = ht.assign_batch(boxes_dev, p0["heatmap"], gt_boxes, gt_labels, n_gt, tc["point_cloud_range"],
                                                   head.assign_weights)
    cls_sum = box_sum = 0.0
    ties = False
    heat, num_pos, miou = [], 0, []
    code_w = np.array(tc["code_weights"])
    for b, (gb, gl) in enumerate(gts):
        boxes = ho.bbox_decode(res["center"][b], res["height"][b], res["dim"][b], res["rot"][b], res["vel"][b],
                               tc["point_cloud_range"], 8, tc["voxel_size"])
        np.testing.assert_allclose(boxes, boxes_dev[b].cpu().numpy(), rtol=1e-5, atol=1e-5)
        t = ho.get_targets_single(gb.numpy(), gl.numpy(), boxes, res["heatmap"][b], cfg,
                                  cost_override=cost_dev[b, :, :len(gb)].cpu().numpy())
        if not np.array_equal(assigned_dev[b].cpu().numpy(), t["assigned"]):  # equal-cost alternatives only
            cd = cost_dev[b, :, :len(gb)].double().cpu().numpy()
            a_dev, a_ref = assigned_dev[b].cpu().numpy(), t["assigned"]
            tot = lambda a: sum(cd[p, a[p] - 1] for p in np.nonzero(a > 0)[0])  # noqa: E731
            assert abs(tot(a_dev) - tot(a_ref)) <= 1e-9 * max(1.0, abs(tot(a_ref))), "device assignment is not optimal"
            ties = True
        num_pos += t["num_pos"]
        miou.append(t["matched_iou"])
        heat.append(t["heatmap"])
        cls_sum += ho.sigmoid_focal_loss(res["heatmap"][b].T, t["labels"], t["label_weights"])
        pred_code = np.concatenate([res[k][b] for k in ("center", "height", "dim", "rot", "vel")], 0).T
        box_sum += ho.l1_loss(pred_code, t["bbox_targets"], t["bbox_weights"] * code_w)
    heat = np.stack(heat)
    assert heat.shape[1] == head.num_classes
    ref_heat = ho.gaussian_focal_loss(ho.clip_sigmoid(res["dense_heatmap"]), heat, avg_factor=max((heat == 1).sum(), 1))
    assert float(losses["loss_heatmap"]) == pytest.approx(ref_heat, rel=rel)
    print("loss terms (device / oracle):", float(losses["layer_-1_loss_cls"]), cls_sum / max(num_pos, 1),
          float(losses["layer_-1_loss_bbox"]), 0.25 * box_sum / max(num_pos, 1), float(losses["matched_ious"]), float(np.mean(miou)))
    if ties:  # an equally optimal matching pairs different boxes: the query losses are compared loosely
        rel = 5e-2
    assert float(losses["layer_-1_loss_cls"]) == pytest.approx(cls_sum / max(num_pos, 1), rel=rel)
    assert float(losses["layer_-1_loss_bbox"]) == pytest.approx(0.25 * box_sum / max(num_pos, 1), rel=rel)
    assert float(losses["matched_ious"]) == pytest.approx(float(np.mean(miou)), abs=2e-4 if not ties else 2e-2)


def test_custom_head_loss_matches_oracle_and_predicts(dev):
    """The real TransFusion loss at 500 proposals and 5 classes (Hungarian 500 x G, velocity code weights 0) against
    oracle/head_oracle.py on the same head outputs; predict() decodes boxes with labels below 5."""
    torch.manual_seed(0)
    model = MODELS.build(custom_data_config(camera=False)).to(dev).train()
    inp = _inputs(dev, 2, camera=False)
    gts = _gts(2)
    feats, _ = model.extract_feat(inp)
    preds = model.bbox_head(feats)
    losses = model.bbox_head.loss_by_feat(preds, gts)
    assert set(losses) == {"loss_heatmap", "layer_-1_loss_cls", "layer_-1_loss_bbox", "matched_ious"}
    total, _ = model.parse_losses(losses)
    assert torch.isfinite(total) and all(torch.isfinite(v).all() for v in losses.values())
    model.bbox_head.check_assignment()
    total.backward()
    for name in ("pts_middle_encoder", "pts_backbone", "pts_neck", "bbox_head"):
        grads = [p.grad for p in getattr(model, name).parameters() if p.requires_grad]
        assert all(g is not None and torch.isfinite(g).all() for g in grads), name
    # velocity code weights 0: the velocity head gets no gradient from the box loss
    vel = model.bbox_head.prediction_heads[0].vel
    assert all(float(p.grad.abs().sum()) == 0.0 for p in vel.parameters())
    _check_losses_against_oracle(model, preds, gts, losses, dev)
    model.eval()
    with torch.no_grad():
        out = model.predict(inp)
    assert len(out) == 2
    for r in out:
        n = r["bboxes_3d"].shape[0]
        assert r["bboxes_3d"].shape == (n, 9) and r["scores_3d"].shape == (n,) and r["labels_3d"].dtype == torch.int32
        assert 0 < n <= 500 and (r["scores_3d"] > 0).all()
        assert (r["labels_3d"] >= 0).all() and (r["labels_3d"] < 5).all()
        assert (r["bboxes_3d"][:, :2].abs() <= 61.2).all()
