"""CPU: the box pairs of tests/iou_cases.py and the fp64 oracle that judges the device on them.  The oracle alone must
reproduce every closed form within 1e-5 (the float32 rounding of yaw + pi, yaw + pi/2 and of the quarter turns is the only
difference, see iou_cases.py), be symmetric, not care where the pair lies, and its 3-D IoU must reduce to the BEV IoU at full
height overlap: the reference stays far inside the 2e-4 the device is held to."""
import numpy as np
import pytest

import iou_cases as ic
from oracle import head_oracle as ho


def test_table_has_every_family_and_enough_seeds():
    assert len(ic.FAMILIES) == 32 and all(ic.SEEDS[n] >= 4 for n in ic.MANY_SEEDS)
    assert {"identical", "yaw_plus_pi", "contained", "concentric_squares_45deg", "far_apart", "axis_aligned"} <= set(ic.CLOSED)
    for name, seed in ic.FAMILY_SEEDS:
        a, b, closed = ic.pairs(name, seed)
        assert a.shape == b.shape == (ic.N, 7) and a.dtype == b.dtype == np.float32
        assert np.isfinite(a).all() and np.isfinite(b).all() and (a[:, 3:6] > 0).all() and (b[:, 3:6] > 0).all()
        assert (np.abs(a[:, 6]) <= np.float32(np.pi)).all() and (np.abs(b[:, 6]) <= np.float32(np.pi)).all()
        assert (closed is not None) == (name in ic.CLOSED)
        h = ic.N // 2
        assert (a[:h, 2] == b[:h, 2]).all() and (a[:, 5] == b[:, 5]).all() and (b[h:, 2] > a[h:, 2]).all()
    assert ic.pairs("generic", 0)[0] is ic.pairs("generic", 0)[0]                       # built once
    assert not np.array_equal(ic.pairs("collinear_overlap", 0)[0], ic.pairs("collinear_overlap", 1)[0])


def test_families_are_what_their_names_say():
    a, b, closed = ic.pairs("collinear_overlap", 0)
    assert (a[:, 6] == b[:, 6]).all() and (a[:, 3:5] == b[:, 3:5]).all() and (closed > 0.02).all() and (closed < 0.91).all()
    for name in ("share_short_edge", "share_long_edge", "share_corner", "collinear_disjoint", "far_apart"):
        for seed in range(ic.SEEDS[name]):
            assert ic.pairs(name, seed)[2].max() < 1e-5, name                          # disjoint up to the rounding of the centres
    a, b, _ = ic.pairs("share_short_edge", 0)
    d = np.linalg.norm(b[:, :2].astype(np.float64) - a[:, :2], axis=1)
    assert (d[::2] >= np.maximum(a[::2, 3], a[::2, 4]) / 2 - 1e-5).all()              # the partner sits beyond the long side's end
    a, b, _ = ic.pairs("axis_aligned", 0)
    assert set(np.unique(np.concatenate([a[:, 6], b[:, 6]]))) == {np.float32(0), np.float32(np.pi / 2), np.float32(np.pi)}
    a, b, _ = ic.pairs("thin_cross", 0)
    assert (a[:, 3] < 1e-4).sum() == ic.N // 2 and (b[:, 4] < 1e-4).sum() == ic.N // 2   # sides below the 1e-4 clamp
    a, b, closed = ic.pairs("axis_aligned", 0)
    assert (closed == 0).any() and ((closed > 0.05) & (closed < 0.95)).any()
    _, iou2d = ic.reference_pairs("generic", 0)
    assert ((iou2d > 0.05) & (iou2d < 0.95)).sum() > ic.N // 2


@pytest.mark.parametrize("name", ic.CLOSED)
def test_oracle_reproduces_the_closed_forms(name):
    for seed in range(ic.SEEDS[name]):
        a, b, closed = ic.pairs(name, seed)
        _, iou2d = ic.reference_pairs(name, seed)
        err = np.abs(iou2d - closed)
        assert err.max() <= 1e-5, (name, seed, int(err.argmax()), iou2d[err.argmax()], closed[err.argmax()])


def test_collinear_overlap_is_one_minus_k_over_one_plus_k():
    """The closed form in the construction parameter: k = shift / side, recovered from the rounded boxes; (1 - k) / (1 + k)
    differs from the interval form only by the perpendicular component of the rounding (4e-6 m of 0.3 m at worst)."""
    a, b, closed = ic.pairs("collinear_overlap", 0)
    d = np.linalg.norm(b[:, :2].astype(np.float64) - a[:, :2], axis=1)
    k = d / np.where(np.arange(ic.N) % 2 == 0, a[:, 3], a[:, 4])
    assert (k > 0.05 - 1e-4).all() and (k < 0.95 + 1e-4).all()
    np.testing.assert_allclose(closed, (1 - k) / (1 + k), atol=5e-5, rtol=0)


@pytest.mark.parametrize("name", list(ic.FAMILIES))
def test_oracle_is_symmetric_and_rigid_motion_invariant(name):
    a, b, _ = ic.pairs(name, 0)
    p, q = a[:, ic.BEV].astype(np.float64), b[:, ic.BEV].astype(np.float64)
    _, iou2d = ic.reference_pairs(name, 0)
    np.testing.assert_allclose(ho.box_iou_rotated_pairs(q, p), iou2d, atol=1e-12, rtol=0)
    np.testing.assert_allclose(ho.bbox_overlaps_3d_lidar_pairs(b, a), ic.reference_pairs(name, 0)[0], atol=1e-12, rtol=0)
    th, t = 0.7312, np.array([3.25, -1.5])
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    for m in (p, q):
        m[:, :2] = m[:, :2] @ rot.T + t
        m[:, 4] += th
    np.testing.assert_allclose(ho.box_iou_rotated_pairs(p, q), iou2d, atol=1e-9, rtol=0)


@pytest.mark.parametrize("name", list(ic.FAMILIES))
def test_3d_iou_reduces_to_bev_iou_at_full_height(name):
    a, b, _ = ic.pairs(name, 0)
    iou3d, _ = ic.reference_pairs(name, 0)
    clamp = lambda m: np.concatenate([m[:, :2], np.clip(m[:, 2:4], 1e-4, None), m[:, 4:]], 1)  # noqa: E731  base_box3d.py:566
    bev = ho.box_iou_rotated_pairs(clamp(a[:, ic.BEV].astype(np.float64)), clamp(b[:, ic.BEV].astype(np.float64)))
    h = ic.N // 2
    # a side below the clamp enters the BEV areas clamped and the volumes as it is: no reduction there (thin_cross only)
    plain = (a[:, 3:5].min(1) >= 1e-4) & (b[:, 3:5].min(1) >= 1e-4)
    assert plain.all() or name == "thin_cross"
    np.testing.assert_allclose(iou3d[:h][plain[:h]], bev[:h][plain[:h]], atol=1e-12, rtol=0)
    pos = (bev[h:] > 0) & plain[h:]
    assert (iou3d[h:][pos] > 0).all() and (iou3d[h:][pos] < bev[h:][pos]).all()
    assert (iou3d[h:][bev[h:] == 0] == 0).all()
    assert (iou3d >= 0).all() and (iou3d <= 1 + 1e-12).all()


@pytest.mark.parametrize("seed", range(4))
def test_hungarian_scene_has_a_clear_optimum(seed):
    pred, gt, labels, logits, expect = ic.hungarian_scene(seed)
    n = len(pred)
    assert n >= ic.N // 2 and len(gt) == 2 * n
    assigned, mo, lab, cost, iou = ho.hungarian_assign(pred, gt, labels, logits, [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], **ic.HUNGARIAN_W)
    np.testing.assert_array_equal(assigned, expect + 1)                    # every prediction takes its moved copy ...
    np.testing.assert_allclose(mo, 0.15 / 1.85, atol=1e-5)
    assert (iou[np.arange(n), np.arange(n)] < 1e-5).all()                 # ... whose touching neighbour has IoU 0 ...
    fav = ho.focal_loss_cost(logits.T, labels, weight=0.5)
    np.testing.assert_allclose(fav[:, 0] - fav[:, n], -0.05, atol=2e-3)    # ... and the better class cost
    margin = ic.assignment_margin(cost)
    assert 0.01 <= margin <= 0.15 / 1.85 - 0.048


def test_pair_helpers_are_the_diagonal_of_the_tables():
    a, b, _ = ic.pairs("generic", 0)
    np.testing.assert_array_equal(ic.reference_table("generic", 0).diagonal(), ic.reference_pairs("generic", 0)[0])
    np.testing.assert_array_equal(ho.box_iou_rotated(a[:9, ic.BEV], b[:9, ic.BEV]).diagonal(), ic.reference_pairs("generic", 0)[1][:9])
