"""GPU: the assembled BEVFusion graph (reference nuScenes config shapes) runs forward + backward through the
HIP operators; shapes as the reference documents them (BF/bevfusion.py:371-381, BF/sparse_encoder.py:151)."""
import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import synthetic
from bevfusion_amd.bevfusion import BEVFusion, nuscenes_config, surrogate_loss
from bevfusion_amd.registry import MODELS

pytestmark = pytest.mark.gpu


def _inputs(dev, B, camera=True, train_aug=True):
    d = {"points": [torch.from_numpy(synthetic.lidar_sweep(40000, seed=1000 + i)).to(dev) for i in range(B)]}
    if camera:
        rig = synthetic.camera_rig(batch=B, seed=1, train_aug=train_aug)
        d["imgs"] = torch.randn(B, 6, 3, 256, 704, device=dev)
        for src, dst in (("lidar2image", "lidar2img"), ("camera_intrinsics", "cam2img"), ("camera2lidar", "cam2lidar"),
                         ("img_aug_matrix", "img_aug_matrix"), ("lidar_aug_matrix", "lidar_aug_matrix")):
            d[dst] = torch.from_numpy(rig[src]).to(dev)
    return d


def test_registry_names():
    for name in ("BEVFusion", "DepthLSSTransform", "LSSTransform", "BEVFusionSparseEncoder", "SubMConv3d", "SparseConv3d",
                 "ConvFuser", "SECOND", "SECONDFPN", "GeneralizedLSSFPN", "BEVFusionHead", "TransformerDecoderLayer"):
        assert name in MODELS, name


def test_lidar_only_forward_backward(dev):
    """BASELINE config 1: hard voxelization + 4-stage sparse encoder (+ BEV backbone/head), fp32."""
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config(camera=False, lidar=True)).to(dev).train()
    outs, _ = model(_inputs(dev, 2, camera=False))
    res = outs[0][0]
    assert res["dense_heatmap"].shape == (2, 10, 180, 180)
    assert res["center"].shape == (2, 2, 200) and res["heatmap"].shape == (2, 10, 200)
    surrogate_loss(outs).backward()
    enc = model.pts_middle_encoder
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in enc.parameters())
    assert enc.conv_input[0].weight.grad.abs().sum() > 0


def test_full_model_forward_backward_bf16(dev):
    """BASELINE config 3 at B=1: camera + LiDAR + fusion + head, bf16 autocast with fp32 index paths."""
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config()).to(dev).train()
    n_params = sum(p.numel() for p in model.parameters())
    assert 34e6 < n_params < 40e6, n_params  # 36.4 M with ResNet-50
    inp = _inputs(dev, 1)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feats, depth_loss = model.extract_feat(inp)
        assert feats[0].shape == (1, 512, 180, 180)
        outs = model.bbox_head(feats)
        loss = surrogate_loss(outs, depth_loss)
    assert torch.isfinite(loss)
    loss.backward()
    for name in ("img_backbone", "view_transform", "pts_middle_encoder", "fusion_layer", "pts_backbone", "bbox_head"):
        grads = [p.grad for p in getattr(model, name).parameters() if p.requires_grad]
        assert all(g is not None and torch.isfinite(g).all() for g in grads), name
    assert model.view_transform.depthnet[0].weight.grad.abs().sum() > 0


def test_side_stream_matches_single_stream(dev):
    """LiDAR branch on a second HIP stream (overlapping the camera branch): its features and, through autograd, its
    gradients are bit-identical to the single-stream run.  (The MIOpen bf16 image backbone is not bit-reproducible
    run to run -- tools/side_dbg.py -- so the comparison is made on the deterministic LiDAR branch.)"""
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config()).to(dev).train()
    inp = _inputs(dev, 1)
    captured = {}
    hook = model.pts_middle_encoder.register_forward_hook(lambda m, i, o: captured.__setitem__("pts", o))
    weight = torch.randn(1, 256, 180, 180, device=dev)
    results = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        model.extract_feat(inp)  # learns the LiDAR branch's row capacities: both runs below take the static (sync-free) path
    for side in (False, True):
        model.lidar_side_stream = side
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            feats, _ = model.extract_feat(inp)
        pts = captured["pts"]
        (pts * weight).sum().backward(retain_graph=False)
        torch.cuda.synchronize()
        enc = model.pts_middle_encoder
        results.append((pts.detach().clone(), enc.conv_input[0].weight.grad.clone(), enc.conv_out[0].weight.grad.clone(),
                        enc.encoder_layers[1][0].norm2.weight.grad.clone()))
        assert feats[0].shape == (1, 512, 180, 180)
    hook.remove()
    assert model._side_stream is not None
    for a_, b_ in zip(*results):
        assert torch.equal(a_, b_)


def test_head_loss_matches_oracle_and_trains(dev):
    """BEVFusion.loss with the real TransFusion targets: every loss term against oracle/head_oracle.py on
    the very same head outputs; backward reaches the head, the BEV backbone and the sparse encoder."""
    import numpy as np
    from bevfusion_amd import head_targets as ht
    from oracle import head_oracle as ho
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config(camera=False, lidar=True)).to(dev).train()
    inp = _inputs(dev, 2, camera=False)
    gts = [tuple(torch.from_numpy(a) for a in synthetic.gt_boxes(seed=3000 + i)) for i in range(2)]
    feats, _ = model.extract_feat(inp)
    preds = model.bbox_head(feats)
    losses = model.bbox_head.loss_by_feat(preds, gts)
    assert set(losses) == {"loss_heatmap", "layer_-1_loss_cls", "layer_-1_loss_bbox", "matched_ious"}
    total, log_vars = model.parse_losses(losses)
    # BF/bevfusion.py:88-121: log_vars carries every entry's mean plus the total under "loss"; matched_ious is logged, not summed
    assert set(log_vars) == set(losses) | {"loss"} and torch.equal(log_vars["loss"], total.detach())
    assert abs(float(total) - sum(float(losses[k].mean()) for k in losses if "loss" in k)) < 1e-4 * abs(float(total))
    assert torch.isfinite(total)
    total.backward()
    for name in ("pts_middle_encoder", "pts_backbone", "pts_neck", "bbox_head"):
        grads = [p.grad for p in getattr(model, name).parameters() if p.requires_grad]
        assert all(g is not None and torch.isfinite(g).all() for g in grads), name
    assert sum(float(p.grad.abs().sum()) for p in model.bbox_head.prediction_heads.parameters()) > 0
    _check_losses_against_oracle(model, preds, gts, losses, dev)


def _check_losses_against_oracle(model, preds, gts, losses, dev, rel=1e-4):
    """Every loss term of BEVFusionHead.loss_by_feat against oracle/head_oracle.py on the very same head outputs."""
    from bevfusion_amd import head_targets as ht
    from oracle import head_oracle as ho
    res = {k: v.detach().float().cpu().numpy() for k, v in preds[0][0].items() if torch.is_tensor(v)}
    tc = model.bbox_head.train_cfg
    cfg = dict(point_cloud_range=tc["point_cloud_range"], voxel_size=tc["voxel_size"], out_size_factor=8,
               grid_size=tc["grid_size"], num_classes=10, code_size=10, gaussian_overlap=0.1, min_radius=2, pos_weight=-1,
               assigner=dict(cls_w=0.15, alpha=0.25, gamma=2.0, reg_w=0.25, iou_w=0.25))
    gt_boxes, gt_labels, n_gt, _ = ht.pack_gt(gts, dev)
    p0 = preds[0][0]
    boxes_dev = model.bbox_head.bbox_coder.decode_boxes(p0["rot"], p0["dim"], p0["center"], p0["height"], p0["vel"])
    assigned_dev, _, cost_dev, _ = ht.assign_batch(boxes_dev, p0["heatmap"], gt_boxes, gt_labels, n_gt, tc["point_cloud_range"],
                                                   model.bbox_head.assign_weights)
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
        same = np.array_equal(assigned_dev[b].cpu().numpy(), t["assigned"])
        if not same:  # equal-cost alternatives only (bf16 head outputs produce exact cost ties): the optimum must agree
            cd = cost_dev[b, :, :len(gb)].double().cpu().numpy()
            a_dev, a_ref = assigned_dev[b].cpu().numpy(), t["assigned"]
            tot = lambda a: sum(cd[p, a[p] - 1] for p in np.nonzero(a > 0)[0])  # noqa: E731
            print("frame", b, "assignment differs in", int((a_dev != a_ref).sum()), "queries; totals", tot(a_dev), tot(a_ref))
            assert abs(tot(a_dev) - tot(a_ref)) <= 1e-9 * max(1.0, abs(tot(a_ref))), "device assignment is not optimal"
            ties = True
        num_pos += t["num_pos"]
        miou.append(t["matched_iou"])
        heat.append(t["heatmap"])
        cls_sum += ho.sigmoid_focal_loss(res["heatmap"][b].T, t["labels"], t["label_weights"])
        pred_code = np.concatenate([res[k][b] for k in ("center", "height", "dim", "rot", "vel")], 0).T
        box_sum += ho.l1_loss(pred_code, t["bbox_targets"], t["bbox_weights"] * code_w)
    heat = np.stack(heat)
    ref_heat = ho.gaussian_focal_loss(ho.clip_sigmoid(res["dense_heatmap"]), heat, avg_factor=max((heat == 1).sum(), 1))
    assert float(losses["loss_heatmap"]) == pytest.approx(ref_heat, rel=rel)
    print("loss terms (device / oracle):", float(losses["layer_-1_loss_cls"]), cls_sum / max(num_pos, 1),
          float(losses["layer_-1_loss_bbox"]), 0.25 * box_sum / max(num_pos, 1), float(losses["matched_ious"]), float(np.mean(miou)))
    if ties:  # an equally optimal matching pairs different boxes: the query losses are compared loosely
        rel = 5e-2
    assert float(losses["layer_-1_loss_cls"]) == pytest.approx(cls_sum / max(num_pos, 1), rel=rel)
    assert float(losses["layer_-1_loss_bbox"]) == pytest.approx(0.25 * box_sum / max(num_pos, 1), rel=rel)
    assert float(losses["matched_ious"]) == pytest.approx(float(np.mean(miou)), abs=2e-4 if not ties else 2e-2)


def test_full_model_batch4_bf16_real_loss_side_stream(dev):
    """The benchmarked configuration (BASELINE configs[3]): batch 4, camera + LiDAR, bf16 autocast with bf16 conv stacks in
    the view transform, LiDAR branch on the side stream, the reference's real TransFusion loss (BEVFusion.loss ->
    BEVFusionHead.loss: Hungarian targets, GaussianFocal + Focal + L1).  Loss terms are checked against head_oracle on
    the same head outputs; backward reaches every sub-module with finite gradients."""
    torch.manual_seed(0)
    B = 4
    model = MODELS.build(nuscenes_config()).to(dev).train()
    model.lidar_side_stream = True
    model.view_transform.conv_dtype = torch.bfloat16
    inp = _inputs(dev, B)
    gts = [tuple(torch.from_numpy(a) for a in synthetic.gt_boxes(seed=3000 + i)) for i in range(B)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feats, _ = model.extract_feat(inp)
        assert feats[0].shape == (B, 512, 180, 180)
        preds = model.bbox_head(feats)
        losses = model.bbox_head.loss_by_feat(preds, gts)
        total, _ = model.parse_losses(losses)
    assert set(losses) == {"loss_heatmap", "layer_-1_loss_cls", "layer_-1_loss_bbox", "matched_ious"}
    assert torch.isfinite(total)
    model.bbox_head.check_assignment()
    total.backward()
    torch.cuda.synchronize()
    for name in ("img_backbone", "img_neck", "view_transform", "pts_middle_encoder", "fusion_layer", "pts_backbone", "pts_neck",
                 "bbox_head"):
        grads = [p.grad for p in getattr(model, name).parameters() if p.requires_grad]
        assert all(g is not None and torch.isfinite(g).all() for g in grads), name
    assert model.view_transform.depthnet[0].weight.grad.abs().sum() > 0
    assert model.pts_middle_encoder.conv_input[0].weight.grad.abs().sum() > 0
    _check_losses_against_oracle(model, preds, gts, losses, dev, rel=2e-4)
    # the same entry point bench.py uses gives the same loss dict keys
    with torch.autocast("cuda", dtype=torch.bfloat16):
        l2 = model.loss(inp, gts)
    assert set(l2) == set(losses)


def test_invalid_matching_cost_poisons_the_loss(dev):
    """A NaN classification logit makes the matching cost invalid: the reference raises from scipy's
    linear_sum_assignment (BF/utils.py:267-270); here the Hungarian kernel flags the frame, every loss term turns NaN
    (visible without a host read) and check_assignment() raises."""
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config(camera=False, lidar=True)).to(dev).train()
    inp = _inputs(dev, 2, camera=False)
    gts = [tuple(torch.from_numpy(a) for a in synthetic.gt_boxes(seed=3000 + i)) for i in range(2)]
    feats, _ = model.extract_feat(inp)
    preds = model.bbox_head(feats)
    good = model.bbox_head.loss_by_feat(preds, gts)
    assert all(torch.isfinite(v) for v in good.values())
    model.bbox_head.check_assignment()
    preds[0][0]["heatmap"] = preds[0][0]["heatmap"].clone()
    preds[0][0]["heatmap"][1, :, 17] = float("nan")   # the cost reads the logits of the GT classes only (BF/utils.py:128-131)
    bad = model.bbox_head.loss_by_feat(preds, gts)
    assert all(torch.isnan(v) for k, v in bad.items() if "loss" in k)
    with pytest.raises(ValueError):
        model.bbox_head.check_assignment()


def test_predict_decodes_boxes(dev):
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config(camera=False, lidar=True)).to(dev).eval()
    with torch.no_grad():
        out = model.predict(_inputs(dev, 2, camera=False))
    assert len(out) == 2
    for r in out:
        n = r["bboxes_3d"].shape[0]
        assert r["bboxes_3d"].shape == (n, 9) and r["scores_3d"].shape == (n,) and r["labels_3d"].dtype == torch.int32
        assert n <= 200 and (r["scores_3d"] > 0).all()
        assert (r["bboxes_3d"][:, :2].abs() <= 61.2).all()


def test_rccl_one_rank_gradient_exchange_on_the_real_parameter_set(tmp_path):
    """Multi-GPU readiness on a one-GPU box: a fresh child process creates a 1-rank `nccl` (= RCCL) group, broadcasts the real
    model's parameters and runs the flat gradient exchange -- plain form and the all-to-all / fp32-sum / all-gather form over
    RCCL -- on the real parameter set (bf16 conv / linear weights with fp32 masters + fp32 rest): gradients come back
    unchanged.  What this cannot show is a second rank; that is the driver's 8-GPU run."""
    import os
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
import bevfusion_amd
from bevfusion_amd.amp import MasterWeightAdamW
from bevfusion_amd.bevfusion import nuscenes_config
from bevfusion_amd.grad_sync import FlatGradAllReduce, broadcast_parameters
from bevfusion_amd.registry import MODELS
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29577", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
torch.cuda.set_device(0)
dist.init_process_group("nccl")
assert dist.get_backend() == "nccl"
torch.manual_seed(0)
model = MODELS.build(nuscenes_config()).cuda().train()
opt = MasterWeightAdamW(model, lr=2e-4, weight_decay=0.01, max_grad_norm=35.0)
before = [p.detach().clone() for p in model.parameters()]
broadcast_parameters(model)
assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
params = [p for p in model.parameters() if p.requires_grad]
g = torch.Generator(device="cuda").manual_seed(1)
for i, p in enumerate(params):
    if i %% 17 != 3:                      # some parameters take no part in the step
        p.grad = torch.randn(p.shape, generator=g, device="cuda", dtype=torch.float32).to(p.dtype).contiguous(
            memory_format=torch.channels_last if p.dim() == 4 else torch.contiguous_format)
want = [None if p.grad is None else p.grad.clone() for p in params]
for form in ("plain", "a2a"):
    os.environ["BFHIP_GRAD_A2A_AT_W1"] = "1" if form == "a2a" else "0"
    gs = FlatGradAllReduce(params)
    assert {str(f.dtype) for _, f, _ in gs.groups} == {"torch.bfloat16", "torch.float32"}
    gs.reduce()
    torch.cuda.synchronize()
    for p, w in zip(params, want):
        if w is None:
            assert p.grad is not None and not p.grad.any()
            p.grad = None
        else:
            assert torch.equal(p.grad, w), form
print("RCCL_ONE_RANK_OK", gs.bytes_per_step())
dist.destroy_process_group()
""" % root
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0 and "RCCL_ONE_RANK_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_camera_only_model_assembly_bf16(dev):
    """BASELINE configs[2] as a model: nuscenes_config(lidar=False) -- ResNet-50 + LSSFPN + DepthLSSTransform (fused
    lift-splat) -> SECOND (80 input channels, no fuser) -> SECONDFPN -> head; forward + real loss + backward in bf16."""
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config(camera=True, lidar=False)).to(dev).train()
    assert model.pts_middle_encoder is None and model.fusion_layer is None
    model.view_transform.conv_dtype = torch.bfloat16
    inp = _inputs(dev, 1)
    gts = [tuple(torch.from_numpy(a) for a in synthetic.gt_boxes(seed=3000))]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        feats, _ = model.extract_feat(inp)
        assert feats[0].shape == (1, 512, 180, 180)
        losses = model.loss(inp, gts)
        total, log_vars = model.parse_losses(losses)
    assert torch.isfinite(total) and "loss" in log_vars
    total.backward()
    for name in ("img_backbone", "img_neck", "view_transform", "pts_backbone", "pts_neck", "bbox_head"):
        grads = [p.grad for p in getattr(model, name).parameters() if p.requires_grad]
        assert any(g is not None and g.abs().sum() > 0 for g in grads), name
        assert all(g is None or torch.isfinite(g).all() for g in grads), name


def test_optimizer_paths_agree_and_skip_nonfinite_steps(dev, monkeypatch):
    """amp.MasterWeightAdamW, three paths over the same clipped steps: (i) through the torch.optim.AdamW object, (ii) direct calls of
    torch's fused multi-tensor kernels on prepared lists -- bit-identical to (i) --, (iii) the flat three-launch path of
    csrc/optim.hip (bfhip_adamw_step) -- the same fp32 arithmetic with its own reduction order for the gradient norm: master
    weights within 2e-6 relative, bf16 copies within one bf16 step.  A step whose gradients are not finite changes nothing in any of
    them (parameters, moments, step counters)."""
    import copy
    from bevfusion_amd.amp import MasterWeightAdamW
    torch.manual_seed(0)
    base = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), torch.nn.BatchNorm2d(16), torch.nn.Conv2d(16, 8, 1),
                               torch.nn.Flatten(), torch.nn.Linear(8 * 6 * 6, 5)).to(dev).to(memory_format=torch.channels_last)
    g = torch.Generator(device=dev).manual_seed(1)
    nets, opts = [], []
    for flat, direct in (("1", "1"), ("0", "1"), ("0", "0")):
        monkeypatch.setenv("BFHIP_FLAT_ADAMW", flat)
        monkeypatch.setenv("BFHIP_DIRECT_ADAMW", direct)
        net = copy.deepcopy(base)
        nets.append(net)
        opts.append(MasterWeightAdamW(net, lr=1e-2, weight_decay=0.01, max_grad_norm=0.5, exclude=()))
    assert opts[0].flat and opts[1].direct and not (opts[2].flat or opts[2].direct)
    for step in range(6):
        grads = [torch.randn(p.shape, generator=g, device=dev) * (3.0 if step % 2 else 0.01) for p in nets[0].parameters()]
        if step == 3:
            grads[0][0, 0, 0, 0] = float("nan")
        if step == 4:
            grads[2] = None                         # a parameter that took no part in the step: zero gradient in every path
        before = [[p.detach().clone() for p in net.parameters()] for net in nets]
        for net, opt in zip(nets, opts):
            opt.zero_grad()
            for p, gr in zip(net.parameters(), grads):
                if gr is not None:
                    p.grad = gr.to(p.dtype).clone(memory_format=torch.preserve_format)
            opt.step()
        for a, b in zip(nets[1].parameters(), nets[2].parameters()):
            assert torch.equal(a, b), step
        for a, b in zip(opts[0].master, opts[2].master):     # fp32 masters of the bf16 parameters
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-7), (step, float((a - b).abs().max()))
        for a, b in zip(nets[0].parameters(), nets[2].parameters()):
            tol = 1e-5 if a.dtype == torch.float32 else 2 ** -7
            assert torch.allclose(a.float(), b.float(), rtol=tol, atol=1e-7), step
        for net, bef in zip(nets, before):
            changed = any(not torch.equal(a, p.detach()) for a, p in zip(bef, net.parameters()))
            assert changed == (step != 3), step
    assert float(opts[1]._steps_flat[0]) == 5.0 and float(opts[0].scalars[2]) == 5.0   # the skipped step did not count
    assert float(opts[0].scalars[1]) == 0.0 and float(opts[0].scalars[5]) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16_autocast"])
def test_prediction_heads_as_row_gemms_match_the_conv1d_stacks(dev, monkeypatch, amp):
    """SeparateHead (centerpoint_head.py:54-82: Conv1d(k=1) -> BN1d -> ReLU -> Conv1d(k=1) per head) evaluated as GEMMs over the
    [B*L, C] rows with the fused row BatchNorm against the same module's Conv1d path: outputs, input gradient, parameter
    gradients and running statistics (fp32: 1e-5; under bf16 autocast: bf16 rounding of the GEMM outputs)."""
    import copy
    from bevfusion_amd import dense_modules as dm
    torch.manual_seed(5)
    heads = dict(center=(2, 2), height=(1, 2), dim=(3, 2), rot=(2, 2), vel=(2, 2), heatmap=(10, 2))
    a = dm.SeparateHead(128, heads).to(dev).train()
    b = copy.deepcopy(a)
    q = torch.randn(4, 200, 128, device=dev)                     # the decoder's [B, L, C] output ...
    xa = q.clone().requires_grad_(True)
    xb = q.clone().requires_grad_(True)
    outs = []
    for mod, x, rows in ((a, xa, True), (b, xb, False)):
        monkeypatch.setattr(dm, "_HEAD_ROWS", rows)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            res = mod(x.transpose(1, 2))                        # ... handed over as [B, C, L]
        assert all(res[h].shape == (4, heads[h][0], 200) for h in heads)
        sum((res[h].float() * (i + 1)).sum() for i, h in enumerate(heads)).backward()
        outs.append(res)
    tol = dict(rtol=2e-2, atol=2e-2) if amp else dict(rtol=1e-4, atol=1e-5)
    for h in heads:
        assert torch.allclose(outs[0][h].float(), outs[1][h].float(), **tol), h
    assert torch.allclose(xa.grad, xb.grad, rtol=5e-2 if amp else 1e-4, atol=5e-2 if amp else 1e-5)
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        scale = float(pb.grad.abs().max()) + 1e-12
        assert float((pa.grad - pb.grad).abs().max()) <= (3e-2 if amp else 1e-4) * scale, n
    for (n, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        if "num_batches" not in n:
            assert torch.allclose(ba, bb, rtol=1e-2 if amp else 1e-4, atol=1e-3 if amp else 1e-6), n


def test_bench_restored_step_repeats():
    """bench.py --dump-outputs restores the state the workload was built with before its last timed step (_InitialState:
    parameters and buffers, MasterWeightAdamW's fp32 masters, moments and device step counter behind its flat tables, the
    transposed weight copies, random number generators, dropout seeds).  Two restored steps of the benchmarked workload, after
    different numbers of training steps, give the same loss and the same gradients: the backward sums in a fixed order (the
    head's proposal rows, the ResNet-50 data gradients).  Only the weight gradients of the layers whose weight gradient is the
    library's may differ, in the last bits of their fp32 sums; the weights after the step may differ where those gradients'
    signs do, by up to two AdamW steps (lr 2e-4)."""
    import os
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = """
import sys, torch
sys.path.insert(0, %r)
import bench
LIB = {"img_backbone.conv1.weight", "view_transform.dtransform.3.weight", "view_transform.depthnet.6.weight",
       "pts_neck.deblocks.1.0.weight", "bbox_head.heatmap_head.1.weight"}
wl = bench.FullModel(torch.device("cuda:0"), 4, 40000)
init = bench._InitialState(wl.model, wl.opt)
runs = []
for r in range(2):
    for _ in range(2 + r):
        wl.step()
    init.restore()
    loss = wl.step()
    torch.cuda.synchronize()
    runs.append((float(loss), {n: (p.grad.detach().float().cpu(), p.detach().float().cpu())
                               for n, p in wl.model.named_parameters() if p.grad is not None}))
(l0, a), (l1, b) = runs
assert l0 == l1, (l0, l1)
assert a.keys() == b.keys() and len(a) > 300, (len(a), len(b))
for n in a:
    (ga, pa), (gb, pb) = a[n], b[n]
    if n in LIB:   # an fp32 sum in another order, rounded to the gradient's dtype (bf16: up to one ulp of the element)
        assert ((ga - gb).abs() <= 2 ** -7 * gb.abs() + 1e-3 * gb.abs().max()).all(), n
        assert torch.allclose(pa, pb, rtol=2 ** -7, atol=4.5e-4), n
    else:
        assert torch.equal(ga, gb), n
        assert (pa - pb).abs().max() <= 1e-6, n
print("RESTORED_STEP_OK", l0)
""" % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and "RESTORED_STEP_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
