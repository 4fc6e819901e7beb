"""GPU: predict() without host reads.  (a) bfhip_predict_compact against its definition head_targets.torch_predict_compact;
(b) the LiDAR branch in eval on static capacities against the exact eval path -- bit for bit: with running statistics no op of
the branch reduces over rows, and an inactive row adds exact zeros to every gather; (c) two consecutive
predict(packed=True) calls under torch.cuda.set_sync_debug_mode("error"), equal to the exact list path; (d) the sparse
BatchNorms in eval on the torch fallback; (e) overflow: flagged in the same forward, in bounds, finite, reported by to_list();
(f) NMS configurations stay on the list path."""
import warnings

import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import bn2d, synthetic
from bevfusion_amd.bevfusion import nuscenes_config
from bevfusion_amd.head_targets import PackedPredictions, predict_compact, torch_predict_compact
from bevfusion_amd.registry import MODELS

from test_predict_pack_cpu import PATTERNS, RANGE, THRESHOLDS, case, same

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ (a) the kernel
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("W", [7, 9])
@pytest.mark.parametrize("P", [1, 200, 500, 4096])
def test_kernel_is_torch_predict_compact(dev, P, W, pattern):
    boxes, heatmap = case(P, W, pattern)
    scores, labels = heatmap.max(1)
    for threshold in THRESHOLDS:
        want = torch_predict_compact(boxes, scores, labels, RANGE, threshold)
        got = predict_compact(boxes.to(dev), scores.to(dev), labels.to(dev), RANGE, threshold)
        for name, g, w in zip(("boxes", "scores", "labels", "counts"), got, want):
            assert same(g.cpu(), w), (name, threshold)
        on_dev = torch_predict_compact(boxes.to(dev), scores.to(dev), labels.to(dev), RANGE, threshold)
        assert all(same(g, w) for g, w in zip(got, on_dev)), threshold


def test_kernel_rejects_what_it_cannot_hold(dev):
    boxes, heatmap = case(200, 7, "all")
    scores, labels = heatmap.max(1)
    with pytest.raises(RuntimeError, match="predict_compact"):
        predict_compact(boxes[..., :6].contiguous().to(dev), scores.to(dev), labels.to(dev), RANGE, None)
    big = torch.zeros(1, 4097, 7, device=dev)
    with pytest.raises(RuntimeError, match="predict_compact"):
        predict_compact(big, big[..., 0].contiguous(), big[..., 0].long(), RANGE, None)


# ------------------------------------------------------------------------------------------ the model
def frames(dev, n_points, seeds):
    return {"points": [torch.from_numpy(synthetic.lidar_sweep(n_points, seed=s)).to(dev) for s in seeds]}


def build_model(dev):
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config(camera=False, lidar=True)).to(dev).eval()
    model.static_lidar = False
    return model


@pytest.fixture(scope="module")
def state(dev):
    """The LiDAR-only model in eval, two 20 000-point frames, and what the exact path gives for them (its forward also learns
    the capacities); then static mode switched on and warmed up.  Tests leave `static_lidar` True and the capacities alone."""
    model = build_model(dev)
    inp = frames(dev, 20000, (70, 71))
    with torch.no_grad():
        feat = model.extract_pts_feat(inp).clone()
        preds = model.predict(inp)
        assert model.capacity_status() is None
        model.static_lidar = True
        assert model._static_lidar_ready()
        model.predict(inp, packed=True)  # warm-up of the static path (pinned buffers, workspaces)
    torch.cuda.synchronize()
    return dict(model=model, inp=inp, feat=feat, preds=preds)


def test_static_eval_features_are_the_exact_path_bits(dev, state):
    model = state["model"]
    before = bn2d.EVAL_LAUNCHES["fwd"]
    with torch.no_grad():
        got = model.extract_pts_feat(state["inp"])
    assert bn2d.EVAL_LAUNCHES["fwd"] > before  # the sparse BatchNorms ran in csrc/bn_eval.hip
    assert model.capacity_status() is not None and not bool(model.capacity_status())
    assert got.shape == state["feat"].shape and got.dtype == state["feat"].dtype
    assert torch.equal(got, state["feat"])


def assert_same_predictions(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for k in w:
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, k
            assert torch.equal(g[k], w[k]), k  # (b) is bit-identical, so scores and boxes are compared bit for bit as well


def test_packed_predict_makes_no_host_read(dev, state):
    model, inp = state["model"], state["inp"]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            first = model.predict(inp, packed=True)
            second = model.predict(inp, packed=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want = state["preds"]
    assert sum(len(w["scores_3d"]) for w in want) > 0
    for packed in (first, second):
        assert isinstance(packed, PackedPredictions) and len(packed) == 2
        assert packed.overflow is not None and packed.overflow.dim() == 0 and packed.overflow.dtype == torch.bool
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert_same_predictions(packed.to_list(), want)
    # the default is today's list through today's code path, static or not
    with torch.no_grad():
        assert_same_predictions(model.predict(inp), want)


def l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


def test_static_eval_on_the_torch_batchnorm_fallback(dev, state, monkeypatch):
    """BFHIP_BN_EVAL=0: BatchNorm1dAct(rows_dev=) in eval takes its torch expression, still without a host read; against the
    exact path on the kernels within the relative L2 of 1e-4 that tests/test_bn_eval_gpu.py allows an fp32 stack."""
    model = state["model"]
    monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", False)
    before = bn2d.EVAL_LAUNCHES["fwd"]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            got = model.extract_pts_feat(state["inp"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bn2d.EVAL_LAUNCHES["fwd"] == before
    e = l2(got, state["feat"])
    print("static eval, torch BatchNorm fallback: relative L2 %.3g" % e)
    assert e <= 1e-4


def test_overflow_is_flagged_in_bounds_and_reported(dev, monkeypatch):
    from bevfusion_amd import spconv
    model = build_model(dev)
    enc = model.pts_middle_encoder
    small, big = frames(dev, 20000, (70, 71)), frames(dev, 120000, (90, 91))
    with torch.no_grad():
        model.predict(small)                                   # exact: learns the capacities from the small frames
        model.static_lidar = True
        ok = model.predict(small, packed=True)
        assert not bool(ok.overflow)
        # keep the capacities where they are: the stall-free monitors would grow them one forward later
        monkeypatch.setattr(enc._monitor, "poll", lambda: None)
        monkeypatch.setattr(model._voxel_monitor, "poll", lambda: None)
        monkeypatch.setattr(spconv, "VALIDATE", True)          # every gather operand of every launch checked to be in range
        out = model.predict(big, packed=True)
        assert bool(out.overflow)
        assert out.boxes.shape == ok.boxes.shape and out.scores.shape == ok.scores.shape and out.labels.shape == ok.labels.shape
        assert bool(torch.isfinite(out.boxes).all()) and bool(torch.isfinite(out.scores).all())
        with pytest.warns(UserWarning, match="capacity"):
            listed = out.to_list(on_overflow="warn")
        assert [len(r["scores_3d"]) for r in listed] == out.counts.tolist()
        with pytest.raises(RuntimeError, match="capacity"):
            out.to_list(on_overflow="raise")
        after = model.predict(small, packed=True)
        assert not bool(after.overflow)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert_same_predictions(after.to_list(), ok.to_list())


def test_packed_with_nms_raises(dev, state):
    head = state["model"].bbox_head
    cfg = head.test_cfg
    head.test_cfg = dict(cfg or {}, nms_type="circle")
    try:
        with torch.no_grad(), pytest.raises(ValueError, match="nms_type"):
            state["model"].predict(state["inp"], packed=True)
    finally:
        head.test_cfg = cfg
