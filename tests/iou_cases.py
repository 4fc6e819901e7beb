"""Structured box pairs for the rotated IoU of csrc/head.hip (rotated_intersection and its three consumers); numpy only.

`pairs(family, seed)` returns two float32 arrays of LiDAR boxes [N, 7] = (x, y, z_bottom, dx, dy, dz, yaw), row i of the first
paired with row i of the second, and the closed-form BEV IoU of every pair where one exists (else None).  The families are
the geometry a polygon clipper gets wrong and random scenes never contain: identical footprints, boxes that differ by a
rotation of 1e-7 ... 1e-2 rad, boxes that share an edge or a corner, boxes shifted along their own axis (collinear edges),
axis-aligned and axis-snapped boxes, nested, very thin and very large boxes.  `generic` is the control.

ROUNDING FIRST.  A pair is built in fp64, rounded to float32, and only then handed to anyone: the closed forms below are
evaluated on the ROUNDED boxes (in fp64), so the closed form, the fp64 oracle and the device kernel answer the same question.
Rounding a 54 m coordinate moves it by up to 4e-6 m, which on a 0.3 m box is worth 1e-5 of IoU: a closed form written in the
unrounded construction parameters, e.g. (1 - k) / (1 + k), would be off by that much.

CLOSED FORMS.  Two rectangles with the same axes u = (cos yaw, sin yaw), v = (-sin yaw, cos yaw) overlap in the product of
two interval overlaps: with (du, dv) the partner's centre in the first box's frame and (wb, hb) its extents along u and v,
    inter = len([-wa/2, wa/2] & [du - wb/2, du + wb/2]) * len([-ha/2, ha/2] & [dv - hb/2, dv + hb/2])
(`frame_iou`).  A partner turned by pi has the same footprint, one turned by pi/2 has it with the sides swapped.  yaw + pi and
yaw + pi/2 are themselves rounded to float32 (after wrapping into +-pi: 1.2e-7 rad at most), which turns a 12 m box by 7e-7 m at
its ends; the IoU moves by less than 1e-6.  float32(pi/2) and float32(pi) are 4e-8 / 9e-8 away from the quarter turns, the same
order.  Nested: the partner has half the sides and stays inside (sides within a factor 2 of each other, turned by at most
0.3 rad, centre offset at most 8 % of the side), IoU = 1/4.  Two concentric squares at 45 degrees: the octagon has area
2 (sqrt 2 - 1) s^2, IoU = 2 (sqrt 2 - 1) / (2 - 2 (sqrt 2 - 1)) = 1 / sqrt 2.

HEIGHTS.  In every family rows [0, N/2) have the same z and dz in both boxes (the 3-D IoU equals the BEV IoU), rows [N/2, N)
have the partner raised by 0.3 dz (height overlap 0.7 dz), so the volume formula is exercised too.
"""
import functools
import zlib

import numpy as np

from oracle import head_oracle as ho

N = 64
BEV = [0, 1, 3, 4, 6]
DYAWS = ("1e-7", "1e-6", "1e-5", "1e-4", "1e-3", "1e-2")
TOL = 2e-4  # fp32 polygon clipping against the fp64 oracle (header of test_head_gpu.py)


def wrap(yaw):
    return (yaw + np.pi) % (2 * np.pi) - np.pi


def _base(rs, n=N):
    """fp64 boxes: x, y in +-54 m, sides 0.3 - 12 m, yaw in +-pi."""
    xy = rs.uniform(-54, 54, (n, 2))
    wh = rs.uniform(0.3, 12, (n, 2))
    z, dz = rs.uniform(-5, 3, n), rs.uniform(0.5, 4, n)
    yaw = rs.uniform(-np.pi, np.pi, n)
    return np.column_stack([xy, z, wh, dz, yaw])


def _axes(a):
    c, s = np.cos(a[:, 6]), np.sin(a[:, 6])
    return np.stack([c, s], 1), np.stack([-s, c], 1)


def _partner(a, du=0.0, dv=0.0, w=None, h=None, dyaw=0.0):
    """A copy of `a` moved by (du, dv) in a's own frame, with sides (w, h) and yaw + dyaw (wrapped into +-pi)."""
    u, v = _axes(a)
    b = a.copy()
    b[:, :2] += np.asarray(du)[..., None] * u + np.asarray(dv)[..., None] * v
    if w is not None:
        b[:, 3] = w
    if h is not None:
        b[:, 4] = h
    b[:, 6] = wrap(a[:, 6] + dyaw)
    return b


def frame_iou(a, b, swapped=False):
    """BEV IoU of boxes with common axes, evaluated in fp64 on the boxes as given (`swapped`: the partner is turned by a
    quarter, its dx lies along the first box's v)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    u, v = _axes(a)
    d = b[:, :2] - a[:, :2]
    du, dv = (d * u).sum(1), (d * v).sum(1)
    sw = np.broadcast_to(np.asarray(swapped, bool), (len(a),))
    wb, hb = np.where(sw, b[:, 4], b[:, 3]), np.where(sw, b[:, 3], b[:, 4])
    ou = np.clip(np.minimum(a[:, 3] / 2, du + wb / 2) - np.maximum(-a[:, 3] / 2, du - wb / 2), 0, None)
    ov = np.clip(np.minimum(a[:, 4] / 2, dv + hb / 2) - np.maximum(-a[:, 4] / 2, dv - hb / 2), 0, None)
    inter = ou * ov
    return inter / (a[:, 3] * a[:, 4] + b[:, 3] * b[:, 4] - inter)


def _along(a, rs, lo, hi):
    """Shift k * side along the box's own axis: along u in even rows, along v in odd rows."""
    k = rs.uniform(lo, hi, len(a))
    even = np.arange(len(a)) % 2 == 0
    return np.where(even, k * a[:, 3], 0.0), np.where(even, 0.0, k * a[:, 4])


# ---------------------------------------------------------------------------------------------- families
# each builder: RandomState -> (a, b, closed) in fp64, closed = None | constant | callable(a32, b32) -> [N]
def _identical(rs):
    a = _base(rs)
    return a, a.copy(), 1.0


def _yaw_plus_pi(rs):
    a = _base(rs)
    return a, _partner(a, dyaw=np.pi), 1.0


def _yaw_plus_half_pi(rs):
    a = _base(rs)
    return a, _partner(a, w=a[:, 4], h=a[:, 3], dyaw=np.pi / 2), 1.0


def _dyaw(delta, jitter):
    def build(rs):
        a = _base(rs)
        b = _partner(a, dyaw=delta * rs.choice([-1.0, 1.0], N))
        if jitter:
            b[:, :2] += rs.normal(0, 0.05, (N, 2))
            b[:, 3:5] *= 1 + 0.02 * rs.normal(0, 1, (N, 2))
        return a, b, None
    return build


def _share_edge(short):
    def build(rs):
        a = _base(rs)
        other = rs.uniform(0.3, 12, N)                                     # the partner's side across the shared edge
        slide = np.where(np.arange(N) % 2 == 1, rs.uniform(-0.5, 0.5, N), 0.0)  # odd rows: the edges overlap in part only
        across_u = (a[:, 3] >= a[:, 4]) == short                          # the shared edge is perpendicular to u
        du = np.where(across_u, (a[:, 3] + other) / 2, slide * a[:, 3])
        dv = np.where(across_u, slide * a[:, 4], (a[:, 4] + other) / 2)
        return a, _partner(a, du, dv, w=np.where(across_u, other, a[:, 3]), h=np.where(across_u, a[:, 4], other)), frame_iou
    return build


def _share_corner(rs):
    a = _base(rs)
    wb, hb = rs.uniform(0.3, 12, N), rs.uniform(0.3, 12, N)
    sgn = rs.choice([-1.0, 1.0], (N, 2))
    return a, _partner(a, sgn[:, 0] * (a[:, 3] + wb) / 2, sgn[:, 1] * (a[:, 4] + hb) / 2, w=wb, h=hb), frame_iou


def _collinear_overlap(rs):
    """Same yaw and size, shift k * side along the box axis, k in (0.05, 0.95): IoU = (1 - k) / (1 + k) before rounding."""
    a = _base(rs)
    return a, _partner(a, *_along(a, rs, 0.05, 0.95)), frame_iou


def _collinear_other_length(rs):
    a = _base(rs)
    other = rs.uniform(0.3, 12, N)
    k = rs.uniform(0.05, 0.95, N)
    even = np.arange(N) % 2 == 0
    du = np.where(even, k * (a[:, 3] + other) / 2, 0.0)
    dv = np.where(even, 0.0, k * (a[:, 4] + other) / 2)
    return a, _partner(a, du, dv, w=np.where(even, other, a[:, 3]), h=np.where(even, a[:, 4], other)), frame_iou


def _collinear_disjoint(rs):
    a = _base(rs)
    return a, _partner(a, *_along(a, rs, 1.0, 2.0)), frame_iou


def _yaw_pi_collinear(rs):
    a = _base(rs)
    return a, _partner(a, *_along(a, rs, 0.05, 1.5), dyaw=np.pi), frame_iou


def _yaw_half_pi_collinear(rs):
    a = _base(rs)
    return (a, _partner(a, *_along(a, rs, 0.05, 1.5), w=a[:, 4], h=a[:, 3], dyaw=np.pi / 2),
            lambda p, q: frame_iou(p, q, swapped=True))


def _same_yaw_generic_shift(rs):
    a = _base(rs)
    return a, _partner(a, rs.uniform(-1.2, 1.2, N) * a[:, 3], rs.uniform(-1.2, 1.2, N) * a[:, 4]), frame_iou


def _axis_aligned(rs):
    """yaw exactly 0.0, float32(pi/2) or float32(pi) in both boxes (independently); rows cycle through partial overlap, a
    shared edge and a shift along the axis; every second triple of rows is snapped to a 0.25 m grid (exactly shared edges)."""
    a = _base(rs)
    quarter = np.array([0.0, np.float32(np.pi / 2), np.float32(np.pi)], np.float64)
    ia, ib = rs.randint(0, 3, N), rs.randint(0, 3, N)
    a[:, 6] = quarter[ia]
    snap = (np.arange(N) // 3) % 2 == 1
    a[:, [0, 1]] = np.where(snap[:, None], np.round(a[:, [0, 1]] * 4) / 4, a[:, [0, 1]])
    a[:, [3, 4]] = np.where(snap[:, None], np.maximum(np.round(a[:, [3, 4]] * 4) / 4, 0.5), a[:, [3, 4]])
    kind = np.arange(N) % 3
    wb = np.where(kind == 1, np.where(snap, np.maximum(np.round(rs.uniform(0.3, 12, N) * 4) / 4, 0.5), rs.uniform(0.3, 12, N)),
                  a[:, 3])                                                # extents in a's frame
    hb = a[:, 4]
    k = rs.uniform(0.05, 1.5, N)
    du = np.select([kind == 0, kind == 1], [rs.uniform(-1.2, 1.2, N) * a[:, 3], (a[:, 3] + wb) / 2], k * a[:, 3])
    dv = np.select([kind == 0, kind == 1], [rs.uniform(-1.2, 1.2, N) * a[:, 4], 0.0], 0.0)
    du = np.where(snap & (kind != 1), np.round(du * 4) / 4, du)
    dv = np.where(snap, np.round(dv * 4) / 4, dv)
    swapped = (ia + ib) % 2 == 1
    b = _partner(a, du, dv, w=np.where(swapped, hb, wb), h=np.where(swapped, wb, hb))
    b[:, 6] = quarter[ib]
    return a, b, lambda p, q: frame_iou(p, q, swapped=swapped)


def _contained(rs):
    a = _base(rs)
    a[:, 3] = rs.uniform(0.6, 6, N)
    a[:, 4] = a[:, 3] * rs.uniform(0.5, 2, N)
    dyaw = np.where(np.arange(N) % 2 == 0, rs.uniform(-0.3, 0.3, N), 0.0)
    b = _partner(a, rs.uniform(-0.08, 0.08, N) * a[:, 3], rs.uniform(-0.08, 0.08, N) * a[:, 4], w=a[:, 3] / 2, h=a[:, 4] / 2,
                 dyaw=dyaw)
    return a, b, 0.25


def _concentric_squares(rs):
    a = _base(rs)
    a[:, 4] = a[:, 3]
    return a, _partner(a, dyaw=np.pi / 4), 2 * (np.sqrt(2) - 1) / (2 - 2 * (np.sqrt(2) - 1))


def _thin_cross(rs):
    """A 'thin x h' box against a 'w x thin' one around the same point: crossing at 90 degrees (rows 0-3 of every 8) and at
    0.3 rad (rows 4-7).  thin = 3e-4, 1e-4 and, below the 1e-4 clamp of iou3d_lidar, 5e-5 and 2e-5."""
    a = _base(rs)
    thin = np.array([3e-4, 1e-4, 5e-5, 2e-5])[np.arange(N) % 4]
    w = a[:, 3].copy()
    a[:, 3] = thin
    dyaw = np.where((np.arange(N) // 4) % 2 == 0, 0.0, np.pi / 2 - 0.3)
    b = _partner(a, rs.uniform(-0.3, 0.3, N) * w / 2, rs.uniform(-0.3, 0.3, N) * a[:, 4] / 2, w=w, h=thin[::-1].copy(), dyaw=dyaw)
    return a, b, None


def _sliver_vs_box(rs):
    a = _base(rs)
    a[:, 3] = rs.uniform(1e-3, 1e-2, N)
    a[:, 4] = rs.uniform(2, 12, N)
    b = _base(rs)
    b[:, :2] = a[:, :2] + rs.uniform(-1, 1, (N, 2))
    return a, b, None


def _huge_vs_small(rs):
    a = _base(rs)
    a[:, 3], a[:, 4] = 80.0, 60.0
    small = _base(rs)
    b = _partner(a, rs.uniform(-50, 50, N), rs.uniform(-40, 40, N), w=small[:, 3], h=small[:, 4],
                 dyaw=np.where(np.arange(N) % 4 == 0, 0.0, small[:, 6]))
    return a, b, None


def _far_apart(rs):
    a, b = _base(rs), _base(rs)
    r, phi = rs.uniform(20, 60, N), rs.uniform(-np.pi, np.pi, N)   # the longest diagonal is 17 m
    b[:, 0], b[:, 1] = a[:, 0] + r * np.cos(phi), a[:, 1] + r * np.sin(phi)
    return a, b, 0.0


def _generic(rs):
    a = _base(rs)
    b = a.copy()
    b[:, :2] += rs.normal(0, 1, (N, 2))
    b[:, 3:5] *= rs.uniform(0.6, 1.4, (N, 2))
    b[:, 6] = np.where(np.arange(N) % 2 == 0, rs.uniform(-np.pi, np.pi, N), wrap(a[:, 6] + rs.normal(0, 0.15, N)))
    return a, b, None


FAMILIES = dict(identical=_identical, yaw_plus_pi=_yaw_plus_pi, yaw_plus_half_pi_swapped_sides=_yaw_plus_half_pi)
for _d in DYAWS:
    FAMILIES["dyaw_" + _d] = _dyaw(float(_d), False)
for _d in DYAWS:
    FAMILIES["dyaw_" + _d + "_jitter"] = _dyaw(float(_d), True)
FAMILIES.update(share_short_edge=_share_edge(True), share_long_edge=_share_edge(False), share_corner=_share_corner,
                collinear_overlap=_collinear_overlap, collinear_overlap_other_length=_collinear_other_length,
                collinear_disjoint=_collinear_disjoint, yaw_pi_collinear=_yaw_pi_collinear,
                yaw_half_pi_collinear=_yaw_half_pi_collinear, same_yaw_generic_shift=_same_yaw_generic_shift,
                axis_aligned=_axis_aligned, contained=_contained, concentric_squares_45deg=_concentric_squares,
                thin_cross=_thin_cross, sliver_vs_box=_sliver_vs_box, huge_vs_small=_huge_vs_small, far_apart=_far_apart,
                generic=_generic)

# a clipper that mishandles collinear edges does so in 0.5 - 2.5 % of such pairs: one seed of 64 can miss, four rarely do
MANY_SEEDS = ("share_short_edge", "share_long_edge", "share_corner", "collinear_overlap", "collinear_overlap_other_length",
              "collinear_disjoint", "yaw_pi_collinear", "yaw_half_pi_collinear")
SEEDS = {name: (4 if name in MANY_SEEDS else 1) for name in FAMILIES}
CLOSED = tuple(n for n in FAMILIES if not n.startswith("dyaw_") and n not in ("thin_cross", "sliver_vs_box", "huge_vs_small",
                                                                             "generic"))
FAMILY_SEEDS = [(name, seed) for name in FAMILIES for seed in range(SEEDS[name])]


@functools.lru_cache(maxsize=None)
def pairs(family, seed=0):
    """(a, b, closed): float32 [N, 7] LiDAR boxes (read-only) and the closed-form BEV IoU [N] of the rounded pairs, or None."""
    rs = np.random.RandomState((zlib.crc32(family.encode()) + 1000003 * seed) % (2 ** 31))
    a, b, closed = FAMILIES[family](rs)
    b[:, 2], b[:, 5] = a[:, 2], a[:, 5]
    b[N // 2:, 2] += 0.3 * a[N // 2:, 5]
    a, b = a.astype(np.float32), b.astype(np.float32)
    if callable(closed):
        closed = closed(a, b)
    elif closed is not None:
        closed = np.full(N, float(closed))
    for arr in (a, b, closed):
        if arr is not None:
            arr.setflags(write=False)
    return a, b, closed


@functools.lru_cache(maxsize=None)
def reference_pairs(family, seed=0):
    """fp64 oracle on the rounded boxes, row i against row i: (3-D IoU [N], BEV IoU [N]); computed once per session."""
    a, b, _ = pairs(family, seed)
    iou3d = ho.bbox_overlaps_3d_lidar_pairs(a, b)
    iou2d = ho.box_iou_rotated_pairs(a[:, BEV], b[:, BEV])
    iou3d.setflags(write=False)
    iou2d.setflags(write=False)
    return iou3d, iou2d


HUNGARIAN_W = dict(cls_w=0.5, alpha=0.25, gamma=2.0, reg_w=0.0, iou_w=1.0)


@functools.lru_cache(maxsize=None)
def hungarian_scene(seed=0):
    """A matching that a wrong IoU of touching boxes turns over.  Predictions: first boxes of `share_short_edge`.  GT: their
    edge-sharing partners (class 1, IoU 0 with 'their' prediction) and, after them, the same boxes moved by 0.85 of the short
    side across it (class 0, same yaw and height: IoU 0.15 / 1.85 = 0.081).  The logits favour class 1 by 0.05 of cost (focal
    cost at logit 0.3 against logit 0, weight 0.5), so every prediction belongs to its moved copy by 0.031 -- and to its
    touching neighbour as soon as that pair's IoU comes out above 0.031.  Pairs whose boxes overlap another pair's (by the
    oracle) are left out, most-entangled first, so that nothing else competes: the margin is that of a single pair.
    -> (pred [n, 7], gt [2n, 7], gt_labels [2n], logits [2, n], expected gt index per prediction [n])."""
    a, b, _ = pairs("share_short_edge", seed)
    p = a.astype(np.float64)
    along_v = p[:, 3] >= p[:, 4]
    t = _partner(p, np.where(along_v, 0.0, 0.85 * p[:, 3]), np.where(along_v, 0.85 * p[:, 4], 0.0)).astype(np.float32)
    table = ho.bbox_overlaps_3d_lidar(a, np.concatenate([b, t]))
    clash = (table[:, :N] > 0) | (table[:, N:] > 0)
    np.fill_diagonal(clash, False)
    clash = clash | clash.T
    keep = np.ones(N, bool)
    while clash[keep][:, keep].any():
        idx = np.nonzero(keep)[0]
        keep[idx[clash[keep][:, keep].sum(1).argmax()]] = False
    n = int(keep.sum())
    gt = np.concatenate([b[keep], t[keep]])
    labels = np.concatenate([np.ones(n, np.int64), np.zeros(n, np.int64)])
    logits = np.stack([np.zeros(n, np.float32), np.full(n, 0.3, np.float32)])
    return np.ascontiguousarray(a[keep]), gt, labels, logits, np.arange(n) + n


def assignment_margin(cost):
    """Total cost of the best assignment that differs from the optimal one, minus the optimal total: a different assignment
    lacks at least one optimal pair, so it is the cheapest of the problems with one optimal pair forbidden."""
    cost = np.asarray(cost, np.float64)
    rows, cols = ho.linear_sum_assignment(cost)
    best = cost[rows, cols].sum()
    runner = np.inf
    for r, c in zip(rows, cols):
        alt = cost.copy()
        alt[r, c] = 1e9
        rr, cc = ho.linear_sum_assignment(alt)
        runner = min(runner, alt[rr, cc].sum())
    return runner - best


@functools.lru_cache(maxsize=None)
def reference_table(family, seed=0):
    """fp64 oracle, every first box against every second box: 3-D IoU [N, N]."""
    a, b, _ = pairs(family, seed)
    t = ho.bbox_overlaps_3d_lidar(a, b)
    t.setflags(write=False)
    return t
