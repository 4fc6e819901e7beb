"""CPU: the packed form of the head's predictions.  head_targets.torch_predict_compact (the definition of the
bfhip_predict_compact kernel) and PackedPredictions.to_list() against the list path, TransFusionBBoxCoder.decode(filter=True).
The decode kernel itself needs a GPU, so the coder is handed the decoded boxes; everything after them is the code under test."""
import functools
import warnings

import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd.head_targets import PackedPredictions, TransFusionBBoxCoder, torch_predict_compact

RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
NUM_CLASSES = 10
PATTERNS = ("all", "none", "alternating", "edges")
THRESHOLDS = (None, 0.0, 0.1)


@functools.lru_cache(maxsize=None)
def case(P, W, pattern, B=2):
    """boxes f32[B,P,W], heatmap f32[B,C,P] (one non-zero class per proposal, as the head builds it).  Never modified."""
    g = torch.Generator().manual_seed(100 * P + 10 * W + PATTERNS.index(pattern))
    rng = torch.tensor(RANGE)
    boxes = torch.randn(B, P, W, generator=g)
    boxes[..., :3] = rng[:3] + (rng[3:] - rng[:3]) * (0.05 + 0.9 * torch.rand(B, P, 3, generator=g))  # inside
    score = 0.2 + 0.7 * torch.rand(B, P, generator=g)                                                    # above 0.1
    p = torch.arange(P)
    if pattern == "none":
        boxes[..., 0] = 100.0
    elif pattern == "alternating":
        boxes[:, p % 2 == 1, 1] = -70.0
    elif pattern == "edges":
        # rows exactly on a bound of the range are kept, one float beyond it they are not; a NaN centre and a NaN score drop
        # the row; scores at and around the threshold 0.1 (as float32), a zero score
        edge = [(0, rng[0]), (1, rng[4]), (2, rng[2]), (2, rng[5]), (0, torch.nextafter(rng[0], rng[0] - 1)),
                (1, torch.nextafter(rng[4], rng[4] + 1)), (2, float("nan")), (0, float("inf"))]
        for k in range(P):
            axis, v = edge[k % len(edge)]
            if k % 3 != 2:
                boxes[:, k, axis] = v
        t = torch.tensor(0.1)
        svals = [t, torch.nextafter(t, t + 1), torch.nextafter(t, t - 1), torch.tensor(float("nan")), torch.tensor(0.0)]
        for k in range(P):
            if k % 2 == 0:
                score[0, k] = svals[(k // 2) % len(svals)]
            if k % 5 == 0:
                score[1, k] = svals[(k // 5) % len(svals)]
    labels = torch.randint(0, NUM_CLASSES, (B, P), generator=g)
    heatmap = torch.zeros(B, NUM_CLASSES, P)
    heatmap.scatter_(1, labels[:, None, :], score[:, None, :])
    return boxes, heatmap


def list_path(boxes, heatmap, threshold):
    """TransFusionBBoxCoder.decode(filter=True) followed by the packaging of BEVFusionHead.predict_by_feat."""
    coder = TransFusionBBoxCoder([-54.0, -54.0], 8, [0.075, 0.075], post_center_range=RANGE, score_threshold=threshold,
                                 code_size=boxes.shape[2] + 1)
    coder.decode_boxes = lambda *a, **k: boxes
    rets = coder.decode(heatmap, None, None, None, None, None, filter=True)
    return [dict(bboxes_3d=r["bboxes"], scores_3d=r["scores"], labels_3d=r["labels"].int()) for r in rets]


def same(a, b):
    """equal values and dtypes; NaN equals NaN (a kept row may carry NaN outside its centre and score)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))


def check_against_list(packed, want):
    boxes, scores, labels, counts = packed.boxes, packed.scores, packed.labels, packed.counts
    B, P, W = boxes.shape
    assert scores.shape == (B, P) and labels.shape == (B, P) and counts.shape == (B,)
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32
    assert counts.tolist() == [len(w["scores_3d"]) for w in want]
    for i, n in enumerate(counts.tolist()):
        assert bool((boxes[i, n:] == 0).all()) and bool((scores[i, n:] == 0).all()) and bool((labels[i, n:] == -1).all())
    got = packed.to_list()
    assert len(got) == len(want) == len(packed)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w) == ["bboxes_3d", "labels_3d", "scores_3d"]
        for k in w:
            assert same(g[k], w[k]), k


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("W", [7, 9])
@pytest.mark.parametrize("P", [1, 200, 500])
def test_torch_predict_compact_is_the_list_path(P, W, pattern, threshold):
    boxes, heatmap = case(P, W, pattern)
    want = list_path(boxes, heatmap, threshold)
    scores, labels = heatmap.max(1)
    packed = PackedPredictions(*torch_predict_compact(boxes, scores, labels, RANGE, threshold))
    check_against_list(packed, want)
    kept = [len(w["scores_3d"]) for w in want]
    if pattern == "all":
        assert kept == [P, P]
    elif pattern == "none":
        assert kept == [0, 0]
    elif pattern == "alternating":
        assert kept == [(P + 1) // 2] * 2


def test_zero_and_none_thresholds_make_no_score_test():
    """`if self.score_threshold:` -- 0.0 is falsy, so a zero (or NaN) score is kept like with None."""
    boxes, heatmap = case(200, 9, "edges")
    scores, labels = heatmap.max(1)
    a = torch_predict_compact(boxes, scores, labels, RANGE, None)
    b = torch_predict_compact(boxes, scores, labels, RANGE, 0.0)
    c = torch_predict_compact(boxes, scores, labels, RANGE, 0.1)
    assert all(same(u, v) for u, v in zip(a, b))
    assert int(c[3].sum()) < int(a[3].sum())
    assert bool(torch.isnan(a[1]).any()) and not bool(torch.isnan(c[1]).any())


def test_to_list_reports_overflow():
    boxes, heatmap = case(200, 7, "alternating")
    scores, labels = heatmap.max(1)
    parts = torch_predict_compact(boxes, scores, labels, RANGE, None)
    clean = PackedPredictions(*parts, overflow=torch.tensor(False))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert len(clean.to_list()) == 2 and len(PackedPredictions(*parts).to_list("raise")) == 2
    over = PackedPredictions(*parts, overflow=torch.tensor(True))
    with pytest.warns(UserWarning, match="capacity"):
        got = over.to_list()
    with pytest.raises(RuntimeError, match="capacity"):
        over.to_list(on_overflow="raise")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        quiet = over.to_list(on_overflow="ignore")
    assert all(same(g[k], q[k]) for g, q in zip(got, quiet) for k in g)
    with pytest.raises(ValueError):
        over.to_list(on_overflow="maybe")


def test_packed_with_nms_is_refused():
    """The NMS branch stays on the list path: packed=True says so before any device work."""
    from bevfusion_amd.dense_modules import BEVFusionHead
    head = BEVFusionHead.__new__(BEVFusionHead)
    torch.nn.Module.__init__(head)
    head.num_proposals, head.num_classes, head.test_cfg = 4, NUM_CLASSES, dict(nms_type="circle")
    head.query_labels = torch.zeros(1, 4, dtype=torch.long)
    preds = dict(heatmap=torch.zeros(1, NUM_CLASSES, 4), query_heatmap_score=torch.zeros(1, NUM_CLASSES, 4))
    with pytest.raises(ValueError, match="nms_type"):
        head.predict_by_feat([[preds]], packed=True)
