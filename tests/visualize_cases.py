"""Cases shared by tests/test_visualize_cpu.py (the specification's properties) and tests/test_visualize_gpu.py (kernel against
specification, torch.equal).  Everything is built from seeds; a case is (function name, kwargs of numpy inputs)."""
import numpy as np

H_BEV, W_BEV = 12, 16
BEV_KW = dict(xlim=(0, W_BEV), ylim=(0, H_BEV), px_per_m=1)


def rig(n_views, f=20.0, cx=18.5, cy=12.5, shape=(3, 3)):
    """lidar2cam [N, 4, 4] of cameras at the origin looking along the directions 2 pi k / N (k = 0: +x; x_cam = -y, y_cam = -z,
    z_cam = x) and cam2img [N, *shape]."""
    base = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64)
    L = []
    for k in range(n_views):
        a = -2 * np.pi * k / n_views
        rz = np.array([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        L.append(base @ rz)
    K = np.zeros((n_views,) + shape, np.float32)
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = cx, cy, 1
    if shape == (4, 4):
        K[:, 3, 3] = 1
    return np.array(L, np.float32), K


def frames(n_views, H, W, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n_views, H, W, 3)).astype(np.uint8)


def ring_boxes(n, seed, r=(4.0, 14.0), dims=((0.8, 0.8, 0.8), (3.5, 2.0, 2.0))):
    rs = np.random.RandomState(seed)
    ang, rad = rs.uniform(-np.pi, np.pi, n), rs.uniform(r[0], r[1], n)
    return np.concatenate([(rad * np.cos(ang))[:, None], (rad * np.sin(ang))[:, None], rs.uniform(-2.0, 0.5, (n, 1)),
                           rs.uniform(dims[0], dims[1], (n, 3)), rs.uniform(-np.pi, np.pi, (n, 1))], 1).astype(np.float32)


def colors(n, seed=1):
    return np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8)


RED, GREEN = np.array([[255, 0, 0]], np.uint8), np.array([[0, 255, 0]], np.uint8)
FRONT = np.array([[8.0, 0.5, -1.0, 1.5, 3.0, 2.0, 0.3]], np.float32)           # in front of view 0 of any rig
FRONT2 = np.array([[8.5, -0.4, -1.2, 2.5, 2.0, 2.4, -0.2]], np.float32)         # overlaps FRONT on the image


def camera_case(name):
    """kwargs of render_cameras for a named case on 25 x 37 frames."""
    L1, K1 = rig(1)
    base = dict(frames=frames(1, 25, 37), lidar2cam=L1, cam2img=K1, thickness=1.5)
    if name == "front":
        return dict(base, boxes=FRONT, colors=RED)
    if name == "behind":
        return dict(base, boxes=FRONT * np.array([-1, 1, 1, 1, 1, 1, 1], np.float32), colors=RED)
    if name == "n0":
        return dict(base, boxes=np.zeros((0, 7), np.float32), colors=np.zeros((0, 3), np.uint8))
    if name == "nan":
        b = np.concatenate([FRONT, FRONT2], 0)
        b[0, 4], b[1, 6] = np.nan, np.inf
        return dict(base, boxes=b, colors=np.concatenate([RED, GREEN]))
    if name == "across":  # from 2 m behind the camera to 6 m in front of it: clipped at the near plane
        return dict(base, boxes=np.array([[2.0, 1.2, -1.0, 8.0, 1.0, 1.5, 0.05]], np.float32), colors=RED)
    if name == "overlap":
        return dict(base, boxes=np.concatenate([FRONT, FRONT2], 0), colors=np.concatenate([RED, GREEN]))
    if name == "overlap_swapped":
        return dict(base, boxes=np.concatenate([FRONT2, FRONT], 0), colors=np.concatenate([GREEN, RED]))
    if name in ("five_views", "three_views_order", "two_views", "six_views_4x4"):
        N = dict(five_views=5, three_views_order=3, two_views=2, six_views_4x4=6)[name]
        L, K = rig(N, shape=(4, 4) if name == "six_views_4x4" else (3, 4))
        b = ring_boxes(9, seed=N)
        kw = dict(base, frames=frames(N, 25, 37, seed=N), lidar2cam=L, cam2img=K, boxes=b, colors=colors(9))
        if name == "three_views_order":
            kw["cam_order"] = [2, 0, 1]
        return kw
    if name.startswith("scale"):
        L, K = rig(2)
        return dict(base, frames=frames(2, 25, 37, seed=5), lidar2cam=L, cam2img=K, boxes=ring_boxes(8, seed=11), colors=colors(8),
                    scale=int(name[5:]), thickness=2.0)
    raise KeyError(name)


CAMERA_CASES = ["front", "behind", "n0", "nan", "across", "overlap", "overlap_swapped", "five_views", "three_views_order", "two_views",
                "six_views_4x4", "scale1", "scale2", "scale3"]


def segment_box(u0, v0, u1, v1):
    """The box with dy = dz = 0 whose footprint on the BEV_KW canvas is the one segment (u0, v0) - (u1, v1) (v = H_BEV - y)."""
    x0, y0, x1, y1 = u0, H_BEV - v0, u1, H_BEV - v1
    return [(x0 + x1) / 2, (y0 + y1) / 2, 0.0, float(np.hypot(x1 - x0, y1 - y0)), 0.0, 0.0, float(np.arctan2(y1 - y0, x1 - x0))]


def canvas(cells):
    """bool [H_BEV, W_BEV] with the (col, row) pairs of `cells` set."""
    m = np.zeros((H_BEV, W_BEV), bool)
    for c, r in cells:
        m[r, c] = True
    return m


def _rect(c0, c1, r0, r1):
    return [(c, r) for c in range(c0, c1 + 1) for r in range(r0, r1 + 1)]


# name -> (segment ends in canvas pixels, thickness in pixels, the covered (col, row) cells worked out by hand: a pixel's centre
# is (col + 0.5, row + 0.5); it is covered when it lies within thickness / 2 of the segment)
COVERAGE = {
    # row 5's centres are ON the segment, which ends ON the centres of (3, 5) and (10, 5); radius 1: rows 4..6 beside it, and
    # the caps reach exactly the centres of (2, 5) and (11, 5) (distance 1.0: the bound is inclusive)
    "horizontal_even": ((3.5, 5.5, 10.5, 5.5), 2.0, _rect(3, 10, 4, 6) + [(2, 5), (11, 5)]),
    # on the border between columns 7 and 8; radius 1.5: centres at 0.5 and 1.5 (inclusive) -> columns 6..9, rows 2..8; caps:
    # (7.5, 1.5) is sqrt(0.25 + 1) = 1.12 from the end (8, 2.5): in; (6.5, 1.5) is 1.80: out
    "vertical_odd": ((8.0, 2.5, 8.0, 8.5), 3.0, _rect(6, 9, 2, 8) + [(7, 1), (8, 1), (7, 9), (8, 9)]),
    # on the border between rows 5 and 6; radius 1.25: centres at 0.5 in, at 1.5 out; caps: (3.5, 5.5) is 1.118 from (4.5, 6): in
    "horizontal_fractional": ((4.5, 6.0, 9.5, 6.0), 2.5, _rect(4, 9, 5, 6) + [(3, 5), (3, 6), (10, 5), (10, 6)]),
    # from the centre of (4, 3) to the centre of (8, 7); radius 1: col - row = 1 is on the line, 0 and 2 are 0.707 away (in), -1
    # and 3 are 1.414 away (out); the caps reach the four centres at distance exactly 1 from the ends
    "diagonal": ((4.5, 3.5, 8.5, 7.5), 2.0, [(4, 3), (5, 4), (6, 5), (7, 6), (8, 7), (4, 4), (5, 5), (6, 6), (7, 7), (5, 3), (6, 4),
                                            (7, 5), (8, 6), (3, 3), (4, 2), (9, 7), (8, 8)]),
    # a zero-length edge on the centre of (8, 5), radius 1.5: the 3 x 3 block (the diagonal neighbours are 1.414 away)
    "disc_odd": ((8.5, 5.5, 8.5, 5.5), 3.0, _rect(7, 9, 4, 6)),
    # a zero-length edge on the corner shared by (7, 5), (8, 5), (7, 6), (8, 6), radius 1: those four (0.707); the next are 1.58
    "disc_even": ((8.0, 6.0, 8.0, 6.0), 2.0, _rect(7, 8, 5, 6)),
}


def coverage_case(name):
    ends, thickness, _ = COVERAGE[name]
    return dict(points=np.zeros((0, 3), np.float32), boxes=np.array([segment_box(*ends)], np.float32), colors=RED, thickness=thickness,
                **BEV_KW)


def bev_case(name):
    if name == "limits":  # on and just outside each limit, duplicates, a NaN and an infinite point
        e = np.float32(1e-3)
        pts = np.array([[0, 0, 0], [-e, 5, 0], [16 - e, 11.5, 0], [16, 3, 0], [5, -e, 0], [7.5, 12 - e, 0], [7.5, 12, 0], [3.2, 4.7, 0],
                        [3.2, 4.7, 1], [3.9, 4.1, 0], [np.nan, 2, 0], [2, np.nan, 0], [np.inf, 3, 0], [9, 1, np.nan]], np.float32)
        return dict(points=pts, boxes=np.zeros((0, 7), np.float32), colors=np.zeros((0, 3), np.uint8), **BEV_KW)
    if name == "point_size":
        pts = np.array([[0.5, 0.5, 0], [15.5, 11.5, 0], [8.2, 6.3, 0]], np.float32)
        return dict(points=pts, boxes=np.zeros((0, 7), np.float32), colors=np.zeros((0, 3), np.uint8), point_size=2, **BEV_KW)
    if name == "footprint_over_point":
        pts = np.array([[4.5, 6.5, 0], [12.5, 2.5, 0]], np.float32)  # the first lies under the footprint's left edge
        return dict(points=pts, boxes=np.array([[7.0, 6.5, 0, 5.0, 3.0, 1.0, 0.0]], np.float32), colors=GREEN, thickness=1.0, **BEV_KW)
    if name == "cloud":
        rs = np.random.RandomState(3)
        pts = np.concatenate([rs.uniform(-30, 30, (3000, 2)), rs.rand(3000, 3)], 1).astype(np.float32)
        b = ring_boxes(20, seed=4, r=(2.0, 24.0), dims=((1.0, 1.0, 1.0), (6.0, 3.0, 2.0)))
        return dict(points=pts, boxes=b, colors=colors(20), xlim=(-25, 25), ylim=(-20, 20), px_per_m=3, point_size=1)
    raise KeyError(name)


BEV_CASES = ["limits", "point_size", "footprint_over_point", "cloud"]


def trap_case():
    """The overflow trap: a degenerate box (dy = dz = 0: one segment) from a corner 1 mm in front of the near plane and 60 m to
    the side -- it projects about 750 000 pixels left of the frame -- to a corner 10 m ahead, seen by a 12 x 16 camera with the
    real rig's focal length."""
    L, K = rig(1, f=1266.0, cx=8.0, cy=6.0)
    a, b = np.array([0.101, 60.0, 0.0]), np.array([10.0, -0.04, -0.02])
    d = b - a
    box = np.array([[*(a + b) / 2, np.linalg.norm(d[:2]), 0.0, 0.0, np.arctan2(d[1], d[0])]], np.float32)
    box[0, 2] = -0.01
    return dict(frames=frames(1, 12, 16, seed=9), boxes=box, colors=RED, lidar2cam=L, cam2img=K, thickness=1.5, near=0.1)
