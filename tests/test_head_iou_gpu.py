"""GPU: the rotated IoU of csrc/head.hip on structured geometry (tests/iou_cases.py) against the fp64 oracle -- boxes that are
identical, turned by 1e-7 ... 1e-2 rad, share an edge or a corner, are shifted along their own axis, axis-aligned, nested,
thin or huge.  The device function rotated_intersection() is reached the way its three consumers reach it: the IoU table of
assign_batch (matching cost), the assigners and build_targets (max_overlaps / ious), and the suppression decision of the
rotated NMS.  Tolerance: 2e-4 absolute, the one test_head_gpu.py states for fp32 polygon clipping against the fp64 oracle;
tests/test_iou_cases_cpu.py shows that the oracle itself is within 1e-5 of every closed form.

Before rotated_intersection() dropped edge crossings that lie outside either box, 14 of the 48 tests here failed on the
MI355X; the figures are in the docstring of test_pairwise_iou_matches_oracle."""
import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
import iou_cases as ic
from bevfusion_amd import head_targets as ht
from bevfusion_amd import synthetic
from oracle import head_oracle as ho

pytestmark = pytest.mark.gpu
PC = synthetic.NUSC["point_cloud_range"]
VS, OSF = synthetic.NUSC["voxel_size"], 8
TOL = ic.TOL
W = dict(cls_w=0.0, alpha=0.25, gamma=2.0, eps=1e-12, reg_w=0.0, iou_w=1.0)   # what HeuristicAssigner3D passes
FULL_TABLE = ("generic", "collinear_overlap", "share_short_edge")
NMS_FAMILIES = ("share_short_edge", "share_long_edge", "share_corner", "collinear_overlap", "collinear_overlap_other_length",
                "collinear_disjoint", "yaw_pi_collinear", "yaw_half_pi_collinear", "identical", "contained", "generic")


def device_tables(dev, pred, gt):
    """assign_batch as HeuristicAssigner3D calls it (one sample, one class, zero logits), with the nuScenes range."""
    P, G = len(pred), len(gt)
    assigned, iou, cost, status = ht.assign_batch(
        torch.from_numpy(np.ascontiguousarray(pred)).to(dev)[None], torch.zeros(1, 1, P, dtype=torch.float32, device=dev),
        torch.from_numpy(np.ascontiguousarray(gt)).to(dev)[None], torch.zeros(1, G, dtype=torch.int32, device=dev),
        torch.tensor([G], dtype=torch.int32).to(dev), PC, W)
    assert int(status[0]) == 0
    return assigned[0], iou[0], cost[0]


@pytest.mark.parametrize("name", list(ic.FAMILIES))
def test_pairwise_iou_matches_oracle(dev, name):
    """iou[i, i] of row i of the first array (prediction) against row i of the second (GT), every seed of the family.

    On the kernel before the fix (crossings of near-parallel edges accepted wherever t1, t2 fell into [0, 1]) the MI355X gave,
    in pairs beyond 2e-4 of 256 / worst error: share_short_edge 4 / 0.837, share_long_edge 4 / 0.430, collinear_overlap
    8 / 0.327, collinear_overlap_other_length 18 / 0.393, yaw_pi_collinear 2 / 0.023, yaw_half_pi_collinear 10 / 0.083; every
    other family at most 1e-4 (thin_cross; dyaw_1e-5 4.3e-5, the rest below 1.1e-5).  The NMS test below made 3, 3, 7, 7, 2
    and 2 wrong decisions on the same families and the Hungarian test (seeds 0 and 3) matched a prediction to its touching
    neighbour."""
    bad, bad_table, worst = [], [], 0.0
    for seed in range(ic.SEEDS[name]):
        a, b, _ = ic.pairs(name, seed)
        want, _ = ic.reference_pairs(name, seed)
        _, iou_t, cost_t = device_tables(dev, a, b)
        _, swap_t, swap_cost = device_tables(dev, b, a)
        for t, c in ((iou_t, cost_t), (swap_t, swap_cost)):
            assert torch.isfinite(t).all() and float(t.min()) >= 0.0 and float(t.max()) <= 1.0 + TOL, (name, seed)
            assert torch.equal(c, -t), (name, seed)                       # cls_w = reg_w = 0, iou_w = 1: the cost IS -iou
        got, swapped = iou_t.diagonal().cpu().numpy().astype(np.float64), swap_t.diagonal().cpu().numpy().astype(np.float64)
        err = np.maximum(np.abs(got - want), np.abs(swapped - want))
        worst = max(worst, float(err.max()))
        for i in np.nonzero((err > TOL) | (np.abs(got - swapped) > TOL))[0]:
            bad.append(f"{name} seed {seed} pair {i}: got {got[i]:.6f} swapped {swapped[i]:.6f} want {want[i]:.6f}\n"
                       f"    a = {a[i].tolist()}\n    b = {b[i].tolist()}")
        if name in FULL_TABLE and seed == 0:                               # off-diagonal: ordinary geometry, guards the indexing
            table = ic.reference_table(name, 0)
            for what, t, ref in (("table", iou_t, table), ("swapped table", swap_t, table.T)):
                e = np.abs(t.cpu().numpy() - ref)
                worst = max(worst, float(e.max()))
                for i, j in zip(*np.nonzero(e > TOL)):
                    bad_table.append(f"{name} seed 0 {what} [{i}, {j}]: got {float(t[i, j]):.6f} want {ref[i, j]:.6f}")
    print(f"\niou_cases {name}: {len(bad)} of {ic.N * ic.SEEDS[name]} pairs beyond {TOL:g}, worst |device - oracle| = {worst:.3g}")
    assert not bad and not bad_table, "\n".join(bad + bad_table)


def test_assigners_and_targets_see_the_oracle_iou(dev):
    """HeuristicAssigner3D.max_overlaps, and the `ious` of build_targets behind a Hungarian matching on the IoU alone, on
    one collinear_overlap batch."""
    a, b, _ = ic.pairs("collinear_overlap", 0)
    table = ic.reference_table("collinear_overlap", 0)
    labels = torch.zeros(ic.N, dtype=torch.long, device=dev)
    res = ht.HeuristicAssigner3D(dist_thre=100).assign(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), None, labels, None)
    inds, _ = ho.heuristic_assign(a, b, np.zeros(ic.N, np.int64), None, 100.0)
    np.testing.assert_array_equal(res.gt_inds.cpu().numpy(), inds)
    m = inds > 0
    assert m.sum() > ic.N // 2 and (table[m, inds[m] - 1] > 0.02).sum() > ic.N // 2      # mostly the pairs themselves
    np.testing.assert_allclose(res.max_overlaps.cpu().numpy()[m], table[m, inds[m] - 1], atol=TOL, rtol=0)
    assert (res.max_overlaps.cpu().numpy()[~m] == 0).all()

    gtb, gtl = torch.from_numpy(b).to(dev)[None], torch.zeros(1, ic.N, dtype=torch.int32, device=dev)
    assigned, iou, cost, status = ht.assign_batch(torch.from_numpy(a).to(dev)[None], torch.zeros(1, 1, ic.N, device=dev), gtb, gtl,
                                                  torch.tensor([ic.N], dtype=torch.int32).to(dev), PC, W)
    _, _, _, _, ious = ht.build_targets(assigned, iou, gtb, gtl, 10, 10, PC, OSF, VS, -1)
    g = assigned[0].cpu().numpy().astype(np.int64) - 1
    assert int(status[0]) == 0 and (g >= 0).all() and len(set(g.tolist())) == ic.N
    np.testing.assert_allclose(ious[0].cpu().numpy(), np.clip(table[np.arange(ic.N), g], 0, 1), atol=TOL, rtol=0)
    # the matching found on the device's IoU is optimal on the oracle's up to the tolerance of the 2 x 64 entries involved
    rows, cols = ho.linear_sum_assignment(-table)
    assert table[np.arange(ic.N), g].sum() >= table[rows, cols].sum() - 2 * ic.N * TOL


@pytest.mark.parametrize("seed", range(4))
def test_hungarian_is_not_misled_by_touching_boxes(dev, seed):
    """iou_cases.hungarian_scene: the logits favour the edge-sharing neighbour (true IoU 0) by 0.05 of cost, the right GT box
    has IoU 0.081; the oracle's optimum is 0.01 or more ahead of any other assignment (asserted here and in
    test_iou_cases_cpu.py), so the device must find it."""
    pred, gt, labels, logits, expect = ic.hungarian_scene(seed)
    ref, mo, lab, cost, _ = ho.hungarian_assign(pred, gt, labels, logits, PC, **ic.HUNGARIAN_W)
    assert ic.assignment_margin(cost) >= 0.01
    np.testing.assert_array_equal(ref, expect + 1)
    w = ic.HUNGARIAN_W
    a = ht.HungarianAssigner3D(cls_cost=dict(type="mmdet.FocalLossCost", gamma=w["gamma"], alpha=w["alpha"], weight=w["cls_w"]),
                               reg_cost=dict(type="BBoxBEVL1Cost", weight=w["reg_w"]), iou_cost=dict(type="IoU3DCost", weight=w["iou_w"]),
                               iou_calculator=dict(type="BboxOverlaps3D", coordinate="lidar"))
    res = a.assign(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(labels).to(dev),
                   torch.from_numpy(logits).to(dev)[None], dict(point_cloud_range=PC))
    np.testing.assert_array_equal(res.gt_inds.cpu().numpy(), ref)
    np.testing.assert_array_equal(res.labels.cpu().numpy(), lab)
    np.testing.assert_allclose(res.max_overlaps.cpu().numpy(), mo, atol=TOL, rtol=0)


@pytest.mark.parametrize("name", NMS_FAMILIES)
def test_rotate_nms_decides_by_the_oracle_iou(dev, name):
    """The 2-D copy of the IoU in rnms_mask_kernel, one pair per call, scores (0.9, 0.8).  With oracle IoU v the second box is
    dropped at thresh v - 0.02 and kept at v + 0.02 (0.02 = 100 x the IoU tolerance; the errors this guards against are
    0.07 - 0.4).  Both sides for 0.05 <= v <= 0.95, the side that exists for the others, thresh 0.02 for v = 0."""
    scores = torch.tensor([0.9, 0.8], device=dev)
    bad, n_both = [], 0
    for seed in range(ic.SEEDS[name]):
        a, b, _ = ic.pairs(name, seed)
        _, iou2d = ic.reference_pairs(name, seed)
        boxes = torch.from_numpy(np.stack([a[:, ic.BEV], b[:, ic.BEV]], 1)).to(dev)     # [N, 2, 5]
        for i, v in enumerate(iou2d.tolist()):
            checks = [(0.02, [0, 1])] if v == 0.0 else []
            if v >= 0.05:
                checks.append((v - 0.02, [0]))
            if 0.0 < v <= 0.95:
                checks.append((v + 0.02, [0, 1]))
            n_both += len(checks) == 2
            for thresh, want in checks:
                got = ht.rotate_nms(boxes[i], scores, thresh).cpu().tolist()
                if got != want:
                    bad.append(f"{name} seed {seed} pair {i}: oracle IoU {v:.6f}, thresh {thresh:.6f}: kept {got}, want {want}\n"
                               f"    a = {a[i, ic.BEV].tolist()}\n    b = {b[i, ic.BEV].tolist()}")
    print(f"\nrotate_nms {name}: {len(bad)} wrong decisions, {n_both} pairs checked on both sides")
    assert not bad, "\n".join(bad)
