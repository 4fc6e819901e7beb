"""Looking at predictions: 3D boxes drawn on the original camera frames, tiled into one mosaic, and a bird's-eye plot of the
cloud with the box footprints -- the reference's tools/visualize/visualize_bboxes_bevfusion.py and visualize_bev.py, which go
through matplotlib on one host core.

    mosaic = render_cameras(frames, boxes, colors, lidar2cam, cam2img)        # uint8 [rows h, cols w, 3]
    bev = render_bev(points, boxes, colors)                                   # uint8 [H, W, 3]
    mosaic, bev = visualize_sample(meta, frames, points, pred, classes, tracker=Tracker3D())

The bits are DEFINED by the restatement in this file (numpy float32 / int64 for the segment set-up, integer torch on any
device for the pixels); csrc/visualize.hip equals it bit for bit.  BFHIP_VISUALIZE=0 selects the restatement; PATHS counts
the calls each way took.  The kernels take uint8 contiguous device frames (device float32 [n, C >= 2] points), frames of at
most max_dim() pixels a side, a thickness of at most max_thickness() / 16 pixels and scale <= max_scale(); anything else
(CPU tensors, arrays, non-contiguous blocks) takes the restatement, same bits.

Geometry, float32, every product, sum and quotient ONE rounded operation in the order written (nothing fused):
  * box table: x, y, z, dx, dy, dz, c, s per box with c = cos(yaw), s = sin(yaw) evaluated in float64 on the host and rounded
    once (box_table).  The kernels never evaluate a sine: the table is their input.  A box with a non-finite value among
    its first seven entries is not drawn.
  * corners (LiDARInstance3DBoxes.corners, lidar_box3d.py:41-80): unit corner u_k = unravel_index(arange(8), [2, 2, 2])
    [[0, 1, 3, 2, 4, 5, 7, 6]] - (0.5, 0.5, 0); l = (dx ux, dy uy, dz uz); rx = lx c + ly (-s); ry = lx s + ly c;
    p = (rx + x, ry + y, lz + z).
  * camera: q_i = ((L_i0 px + L_i1 py) + L_i2 pz) + L_i3 for the rows i = 0, 1, 2 of lidar2cam.
  * near plane -- a DEPARTURE from the reference, which draws a box as soon as one corner has z_cam > 0 and joins corners
    behind the camera with meaningless lines: every edge is clipped against z_cam = near first.  Both ends below near: the
    edge is dropped.  One end (o) below and the other (i) at or above it: tt = (z_i - near) / (z_i - z_o), the end o
    becomes (x_i + tt (x_o - x_i), y_i + tt (y_o - y_i), near).
  * projection: cam2img given as 3x3, 3x4 or 4x4 (visualize_bboxes_bevfusion.py:144-156) is brought to 3x4 (a zero column
    for 3x3, the first three rows of 4x4); h_i = ((K_i0 qx + K_i1 qy) + K_i2 qz) + K_i3; u = h_0 / h_2, v = h_1 / h_2.  An
    edge with an end whose h_2 is not > 0 is dropped.  The reference's `+ 1e-8` in the divisor is NOT kept: relative to h_2
    >= near it is at most 1e-7 for near = 0.1 and below half a float32 ulp for h_2 >= 0.17; the golden comparison
    (tests/test_visualize_cpu.py) carries it as a term of its bound and passes without it.
  * fixed point: X = rint(16 u) (round to nearest even), 1/16 pixel.  An edge with |X| or |Y| >= 2^29 (2^25 pixels) at
    either end, or a non-finite one, is dropped.  Everything after this line is integer.

Guard rectangle (int64): the segment is clipped to [-G, 16 W + G] x [-G, 16 H + G], G = 2048 (128 pixels), x first, then y,
per axis: end 0 against the low and the high bound, then end 1; the moved end gets b + rdiv((b' - b)(bound - a), a' - a)
along the other axis, rdiv = rounded division, halves up.  |a|, |b| < 2^29 makes every product < 2^60.  G exceeds half the
largest thickness, so the part cut away and the new round cap cover no pixel of the frame.

Coverage (int64, no square root): in units of 1/32 pixel the centre of pixel (col, row) is P = (32 col + 16, 32 row + 16),
the ends are A = 2 (X0, Y0), B = 2 (X1, Y1) and the radius is R = thickness in 1/16 pixel.  With d = B - A, e = P - A,
f = P - B: dot = d.e <= 0 -> covered iff e.e <= R^2 (before the first end; a zero-length edge is a disc); dot >= d.d ->
covered iff f.f <= R^2; otherwise covered iff |cross| < 2^31 and cross^2 <= R^2 d.d, cross = dx ey - dy ex.  Bounds: after
the guard clip every |d|, |e|, |f| component is < 2^19, so dot, d.d, |cross| < 2^39 and R^2 d.d < 2^22 2^39 = 2^61;
|cross| >= 2^31 means cross^2 >= 2^62 > R^2 d.d, not covered, and below it the square fits.  The shape is a capsule, opaque
and not anti-aliased (a departure from matplotlib's anti-aliased Agg lines).  Where several boxes cover a pixel the highest
box index wins: matplotlib's painter order.

Default thicknesses are settings derived from the reference's figures, not measurements.  Camera: linewidth 2 pt at
matplotlib's default 100 dpi is 2 * 100 / 72 = 2.78 figure pixels; each axes is nominally 5 in = 500 figure pixels wide and
shows the W-pixel frame, so the line is 2.78 * W / 500 frame pixels: 8.89 at W = 1600, kept as round(16 * that) / 16.  BEV:
25 pt at dpi = 10 is 25 * 10 / 72 = 3.47 pixels, kept as 56 / 16 = 3.5.

BFHIP_VISUALIZE ships on (measured with tools/visualize_micro.py: DESIGN.md section 6).
"""
import math
import os

import numpy as np
import torch

from . import _lib
from .registry import VISUALIZERS

ENABLED = os.environ.get("BFHIP_VISUALIZE", "1") != "0"
PATHS = {"kernel": 0, "torch": 0}  # calls taken by each path (tests, tools)

OBJECT_PALETTE = {
    "car": (255, 158, 0), "truck": (255, 99, 71), "construction_vehicle": (233, 150, 70), "bus": (255, 69, 0),
    "trailer": (255, 140, 0), "barrier": (112, 128, 144), "motorcycle": (255, 61, 99), "bicycle": (220, 20, 60),
    "pedestrian": (0, 0, 230), "traffic_cone": (47, 79, 79),
}
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
FOOTPRINT = ((0, 3), (3, 7), (7, 4), (4, 0))
UNIT_CORNERS = (np.stack(np.unravel_index(np.arange(8), [2, 2, 2]), 1)[[0, 1, 3, 2, 4, 5, 7, 6]]
                - np.array([0.5, 0.5, 0.0])).astype(np.float32)
GUARD = 2048           # 1/16 pixel: the guard rectangle's margin round the frame
FIX_LIMIT = 1 << 29    # 1/16 pixel: fixed-point ends at or beyond it drop the edge
CROSS_LIMIT = 1 << 31  # |cross| at or above it: not covered, its square is never formed
REC = 8                # int32 words of a segment record: X0, Y0, X1, Y1, col0 | row0 << 16, col1 | row1 << 16, box, thickness
_EMPTY_LO = 1 | (1 << 16)


def max_dim():
    """The longest frame side the kernels take (bfhip_vis_max_dim)."""
    return int(_lib.load().bfhip_vis_max_dim())


def max_thickness():
    """The largest thickness, in 1/16 pixel, the kernels and the coverage bounds take (bfhip_vis_max_thickness)."""
    return int(_lib.load().bfhip_vis_max_thickness())


def max_scale():
    """The largest `scale` the composite kernel takes (bfhip_vis_max_scale)."""
    return int(_lib.load().bfhip_vis_max_scale())


_MAX_DIM, _MAX_T, _MAX_SCALE = 8192, 2048, 4  # the library's limits (tests hold the two together)


# ----------------------------------------------------------------------------------------------------------------- inputs
def _host(a, dtype=None):
    a = getattr(a, "tensor", a)
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


def palette_colors(labels, classes):
    """uint8 [n, 3]: OBJECT_PALETTE of classes[label], white for a name outside it or a label outside `classes`."""
    labels = _host(labels).reshape(-1)
    out = np.full((labels.shape[0], 3), 255, np.uint8)
    for i, lab in enumerate(labels):
        lab = int(lab)
        name = classes[lab] if classes is not None and 0 <= lab < len(classes) else "unknown"
        out[i] = OBJECT_PALETTE.get(name, (255, 255, 255))
    return out


def box_table(boxes):
    """float32 [n, 8]: x, y, z, dx, dy, dz, cos(yaw), sin(yaw) of boxes [n, >= 7]; the cosine and sine are taken in float64
    and rounded once.  A row with a non-finite value among the seven has a non-finite entry here as well."""
    b = _host(boxes)
    if b.ndim != 2 or b.shape[1] < 7:
        if b.size == 0:
            return np.zeros((0, 8), np.float32)
        raise ValueError("boxes must be [n, 7 or more], got %s" % (b.shape,))
    b = b[:, :7].astype(np.float32)
    yaw = b[:, 6].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.ascontiguousarray(np.concatenate([b[:, :6], np.cos(yaw)[:, None].astype(np.float32),
                                                    np.sin(yaw)[:, None].astype(np.float32)], 1))


def _table_corners(tab):
    u = UNIT_CORNERS[None]
    lx, ly, lz = tab[:, None, 3] * u[..., 0], tab[:, None, 4] * u[..., 1], tab[:, None, 5] * u[..., 2]
    c, s = tab[:, None, 6], tab[:, None, 7]
    rx = lx * c + ly * (-s)
    ry = lx * s + ly * c
    return np.stack([rx + tab[:, None, 0], ry + tab[:, None, 1], lz + tab[:, None, 2]], -1)


def box_corners(boxes):
    """float32 [n, 8, 3]: LiDARInstance3DBoxes.corners in the module's operation order."""
    with np.errstate(invalid="ignore", over="ignore"):
        return _table_corners(box_table(boxes))


def _affine(m, p):
    """((m0 p0 + m1 p1) + m2 p2) + m3 for the three rows of m [..., 3, 4] and p [..., 3], float32."""
    return np.stack([((m[..., i, 0] * p[..., 0] + m[..., i, 1] * p[..., 1]) + m[..., i, 2] * p[..., 2]) + m[..., i, 3]
                     for i in range(3)], -1)


def as_cam2img(cam2img):
    """float32 [N, 3, 4] of cam2img given as [N, 3, 3], [N, 3, 4] or [N, 4, 4]."""
    k = _host(cam2img, np.float32)
    if k.ndim != 3 or k.shape[1:] not in ((3, 3), (3, 4), (4, 4)):
        raise ValueError("cam2img must be [N, 3, 3], [N, 3, 4] or [N, 4, 4], got %s" % (k.shape,))
    if k.shape[2] == 3:
        k = np.concatenate([k, np.zeros((k.shape[0], 3, 1), np.float32)], 2)
    return np.ascontiguousarray(k[:, :3, :])


def as_lidar2cam(lidar2cam):
    m = _host(lidar2cam, np.float32)
    if m.ndim != 3 or m.shape[1] not in (3, 4) or m.shape[2] != 4:
        raise ValueError("lidar2cam must be [N, 4, 4] or [N, 3, 4], got %s" % (m.shape,))
    return np.ascontiguousarray(m[:, :3, :])


def project_corners(corners, lidar2cam, cam2img):
    """(uv float32 [N, n, 8, 2], z_cam float32 [N, n, 8]) of corners [n, 8, 3]: the camera transform and the projection with NO
    near-plane clip -- what the reference's project_to_image computes (its `valid` is z_cam > 0)."""
    L, K = as_lidar2cam(lidar2cam), as_cam2img(cam2img)
    with np.errstate(all="ignore"):
        q = _affine(L[:, None, None], np.asarray(corners, np.float32)[None])
        h = _affine(K[:, None, None], q)
        return np.stack([h[..., 0] / h[..., 2], h[..., 1] / h[..., 2]], -1), q[..., 2]


# ------------------------------------------------------------------------------------------------- segment set-up (host)
def _rdiv(num, den):
    """Rounded num / den, halves up, int64 arrays; den != 0."""
    neg = den < 0
    num, den = np.where(neg, -num, num), np.where(neg, -den, den)
    return (2 * num + den) // (2 * den)


def _clip_axis(a0, b0, a1, b1, lo, hi, keep):
    keep = keep & ~(((a0 < lo) & (a1 < lo)) | ((a0 > hi) & (a1 > hi)))
    for bound, below in ((lo, True), (hi, False)):
        need = keep & ((a0 < bound) if below else (a0 > bound))
        den = np.where(need, a1 - a0, 1)
        b0 = np.where(need, b0 + _rdiv((b1 - b0) * (bound - a0), den), b0)
        a0 = np.where(need, bound, a0)
    for bound, below in ((lo, True), (hi, False)):
        need = keep & ((a1 < bound) if below else (a1 > bound))
        den = np.where(need, a0 - a1, 1)
        b1 = np.where(need, b1 + _rdiv((b0 - b1) * (bound - a1), den), b1)
        a1 = np.where(need, bound, a1)
    return a0, b0, a1, b1, keep


def _records(u0, v0, u1, v1, keep, box, t, H, W):
    """int32 [..., REC] segment records of float32 pixel ends; `keep` False drops the edge (an empty pixel box)."""
    with np.errstate(all="ignore"):
        q = [np.rint(a * np.float32(16.0)) for a in (u0, v0, u1, v1)]
        for a in q:
            keep = keep & (np.abs(a) < np.float32(FIX_LIMIT))  # a NaN fails
        x0, y0, x1, y1 = [np.where(keep, a, 0).astype(np.int64) for a in q]
    x0, y0, x1, y1, keep = _clip_axis(x0, y0, x1, y1, -GUARD, 16 * W + GUARD, keep)
    y0, x0, y1, x1, keep = _clip_axis(y0, x0, y1, x1, -GUARD, 16 * H + GUARD, keep)
    c0 = np.maximum(-((-(2 * np.minimum(x0, x1) - t - 16)) // 32), 0)
    c1 = np.minimum((2 * np.maximum(x0, x1) + t - 16) // 32, W - 1)
    r0 = np.maximum(-((-(2 * np.minimum(y0, y1) - t - 16)) // 32), 0)
    r1 = np.minimum((2 * np.maximum(y0, y1) + t - 16) // 32, H - 1)
    keep = keep & (c0 <= c1) & (r0 <= r1)
    rec = np.zeros(keep.shape + (REC,), np.int32)
    for i, a in enumerate((x0, y0, x1, y1)):
        rec[..., i] = np.where(keep, a, 0)
    rec[..., 4] = np.where(keep, c0 | (r0 << 16), _EMPTY_LO)
    rec[..., 5] = np.where(keep, c1 | (r1 << 16), 0)
    rec[..., 6] = box
    rec[..., 7] = t
    return rec


def camera_segments(table, lidar2cam, cam2img, near, t, H, W):
    """int32 [N, n * 12, REC]: the records of every (camera, box, edge), box-major, as the set-up kernel writes them."""
    L, K = as_lidar2cam(lidar2cam), as_cam2img(cam2img)
    N, n = L.shape[0], table.shape[0]
    if n == 0:
        return np.zeros((N, 0, REC), np.int32)
    near = np.float32(near)
    ea, eb = np.array(EDGES).T
    with np.errstate(all="ignore"):
        finite = np.isfinite(table).all(1)
        q = _affine(L[:, None, None], _table_corners(table)[None])  # [N, n, 8, 3]
        a, b = q[:, :, ea], q[:, :, eb]                              # [N, n, 12, 3]
        za, zb = a[..., 2], b[..., 2]
        ina, inb = za >= near, zb >= near
        keep = finite[None, :, None] & (ina | inb)
        swap = ~ina  # the inner end is b
        pi = np.where(swap[..., None], b, a)
        po = np.where(swap[..., None], a, b)
        tt = (pi[..., 2] - near) / (pi[..., 2] - po[..., 2])
        cx = pi[..., 0] + tt * (po[..., 0] - pi[..., 0])
        cy = pi[..., 1] + tt * (po[..., 1] - pi[..., 1])
        clipped = np.stack([cx, cy, np.broadcast_to(near, cx.shape)], -1)
        a = np.where((~ina & inb)[..., None], clipped, a)
        b = np.where((ina & ~inb)[..., None], clipped, b)
        ha, hb = _affine(K[:, None, None], a), _affine(K[:, None, None], b)
        keep = keep & (ha[..., 2] > 0) & (hb[..., 2] > 0)
        u0, v0, u1, v1 = ha[..., 0] / ha[..., 2], ha[..., 1] / ha[..., 2], hb[..., 0] / hb[..., 2], hb[..., 1] / hb[..., 2]
    box = np.broadcast_to(np.arange(n)[None, :, None], keep.shape)
    return _records(u0, v0, u1, v1, keep, box, t, H, W).reshape(N, n * 12, REC)


def bev_segments(table, x0, y1, px_per_m, t, H, W):
    """int32 [1, n * 4, REC]: the footprint edges, u = (x - x0) px_per_m, v = (y1 - y) px_per_m in float32."""
    n = table.shape[0]
    if n == 0:
        return np.zeros((1, 0, REC), np.int32)
    x0, y1, ppm = np.float32(x0), np.float32(y1), np.float32(px_per_m)
    ea, eb = np.array(FOOTPRINT).T
    with np.errstate(all="ignore"):
        finite = np.isfinite(table).all(1)
        p = _table_corners(table)
        u, v = (p[..., 0] - x0) * ppm, (y1 - p[..., 1]) * ppm
    keep = np.broadcast_to(finite[:, None], (n, 4))
    box = np.broadcast_to(np.arange(n)[:, None], (n, 4))
    return _records(u[:, ea], v[:, ea], u[:, eb], v[:, eb], keep, box, t, H, W).reshape(1, n * 4, REC)


# ------------------------------------------------------------------------------------------------------ pixels (torch)
def infer_grid(n_views):
    """(rows, cols) of the mosaic: three columns above two views (visualize_bboxes_bevfusion.py:202-206)."""
    cols = 3 if n_views > 2 else n_views
    return int(math.ceil(n_views / max(1, cols))), cols


def _paint(best, rec):
    """Raise best (int32 [H, W]) to the box index wherever a record of rec (host int32 [S, REC]) covers the pixel."""
    dev = best.device
    for x0, y0, x1, y1, lo, hi, box, t in rec[(rec[:, 4] != _EMPTY_LO) | (rec[:, 5] != 0)].tolist():
        c0, r0, c1, r1 = lo & 0xffff, lo >> 16, hi & 0xffff, hi >> 16
        ex = (torch.arange(c0, c1 + 1, dtype=torch.int64, device=dev) * 32 + (16 - 2 * x0))[None, :]
        ey = (torch.arange(r0, r1 + 1, dtype=torch.int64, device=dev) * 32 + (16 - 2 * y0))[:, None]
        dx, dy, r2 = 2 * (x1 - x0), 2 * (y1 - y0), t * t
        len2 = dx * dx + dy * dy
        dot = dx * ex + dy * ey
        fx, fy = ex - dx, ey - dy
        ca = (dx * ey - dy * ex).abs()
        small = ca < CROSS_LIMIT
        cs = torch.where(small, ca, torch.zeros_like(ca))
        cov = torch.where(dot <= 0, ex * ex + ey * ey <= r2,
                          torch.where(dot >= len2, fx * fx + fy * fy <= r2, small & (cs * cs <= r2 * len2)))
        sub = best[r0:r1 + 1, c0:c1 + 1]
        sub.copy_(torch.where(cov, torch.clamp(sub, min=box), sub))


def torch_composite(src, rec, colors, cell_view, rows, cols, scale):
    """The specification of the composite: src uint8 [N, H, W, 3] tensor (any device), rec host int32 [N, S, REC], colors uint8
    [n, 3], cell_view: the view of each mosaic cell (-1 or missing: black) -> uint8 [rows h, cols w, 3] on src's device."""
    N, H, W = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    dev, s = src.device, int(scale)
    h, w = H // s, W // s
    out = torch.zeros((rows * h, cols * w, 3), dtype=torch.uint8, device=dev)
    pal = torch.from_numpy(np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)).to(dev)
    done = {}
    for cell, view in enumerate(list(cell_view)[:rows * cols]):
        if view < 0:
            continue
        if view not in done:
            best = torch.full((H, W), -1, dtype=torch.int32, device=dev)
            _paint(best, rec[view])
            img = src[view]
            if pal.shape[0]:
                img = torch.where((best >= 0)[..., None], pal[best.clamp(min=0).long()], img)
            if s > 1:
                blk = img[:h * s, :w * s].reshape(h, s, w, s, 3).to(torch.int32).sum((1, 3))
                img = ((blk + (s * s) // 2) // (s * s)).to(torch.uint8)
            done[view] = img
        r, c = divmod(cell, cols)
        out[r * h:(r + 1) * h, c * w:(c + 1) * w] = done[view]
    return out


def torch_bev_points(points, x0, y0, px_per_m, point_size, H, W):
    """The specification of the point scatter: uint8 [1, H, W, 3] on the points' device, white point_size squares on black.
    col = floor((x - x0) px_per_m), row = H - 1 - floor((y - y0) px_per_m), float32, one operation each; a point is kept when
    0 <= col < W and 0 <= the floor of y < H (compared as floats, so a NaN or infinite x or y drops the point); the square
    spans [col - (p - 1) // 2, col + p // 2], rows alike, cut at the canvas."""
    dev = points.device
    canvas = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    if points.shape[0]:
        pts = points[:, :2].to(torch.float32).cpu()  # float32 subtract, multiply, floor: the same bits on any device
        fc = torch.floor((pts[:, 0] - np.float32(x0)) * np.float32(px_per_m))
        fr = torch.floor((pts[:, 1] - np.float32(y0)) * np.float32(px_per_m))
        ok = (fc >= 0) & (fc < W) & (fr >= 0) & (fr < H)
        col, row = fc[ok].to(torch.int64).to(dev), (H - 1) - fr[ok].to(torch.int64).to(dev)
        p = int(point_size)
        for dr in range(-((p - 1) // 2), p // 2 + 1):
            for dc in range(-((p - 1) // 2), p // 2 + 1):
                rr, cc = row + dr, col + dc
                m = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
                canvas[rr[m], cc[m]] = 255
    return canvas[None, :, :, None].expand(1, H, W, 3).contiguous()


# ---------------------------------------------------------------------------------------------------------------- kernels
def _upload(dev, *arrays):
    """Device views of ONE buffer of 4-byte words: packed in one pinned host buffer, one non-blocking copy."""
    flat = [np.ascontiguousarray(a).reshape(-1).view(np.int32) for a in arrays]
    sizes = [f.shape[0] for f in flat]
    total = max(sum(sizes), 1)
    host = torch.empty(total, dtype=torch.int32, pin_memory=True)
    if sum(sizes):
        np.concatenate(flat, out=host.numpy()[:sum(sizes)])
    buf = torch.empty(total, dtype=torch.int32, device=dev)
    buf.copy_(host, non_blocking=True)
    out, off = [], 0
    for n in sizes:
        out.append(buf[off:off + n])
        off += n
    return out


def _packed_colors(colors, n):
    c = _host(colors, np.uint8).reshape(-1, 3)
    if c.shape[0] != n:
        raise ValueError("colors must be [%d, 3], got %s" % (n, c.shape))
    return c, (c[:, 0].astype(np.int32) | (c[:, 1].astype(np.int32) << 8) | (c[:, 2].astype(np.int32) << 16))


def _frames_kernel_ok(frames, t, scale):
    return (ENABLED and torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous()
            and 1 <= frames.shape[1] <= _MAX_DIM and 1 <= frames.shape[2] <= _MAX_DIM and 1 <= scale <= _MAX_SCALE
            and frames.shape[1] // scale >= 1 and frames.shape[2] // scale >= 1)


def _as_frames(frames):
    if not torch.is_tensor(frames):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8:
        raise ValueError("frames must be uint8 [N, H, W, 3]")
    return frames


def _thickness_units(thickness, default_px):
    t = int(round(16.0 * (default_px if thickness is None else float(thickness))))
    if not 1 <= t <= _MAX_T:
        raise ValueError("thickness must lie in [1/16, %d] pixels" % (_MAX_T // 16))
    return t


def default_camera_thickness(W):
    """2 pt at 100 dpi on a nominal 500-pixel axes showing W pixels, in pixels (a multiple of 1/16)."""
    return round(16.0 * (2.0 * 100.0 / 72.0) * W / 500.0) / 16.0


DEFAULT_BEV_THICKNESS = 3.5  # 25 pt at dpi = 10 -> 3.47 pixels, as a multiple of 1/16


def _kernel_composite(src, work, nbytes, n, edges, packed, cells, rows, cols, scale):
    N, H, W = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    out = torch.empty((rows * (H // scale), cols * (W // scale), 3), dtype=torch.uint8, device=src.device)
    _lib.call("bfhip_vis_composite", src.data_ptr(), N, H, W, work.data_ptr(), nbytes, n, edges,
              packed.data_ptr() if n else None, cells.data_ptr(), rows, cols, scale, out.data_ptr(), _lib.stream_of(src))
    return out


def render_cameras(frames, boxes, colors, lidar2cam, cam2img, thickness=None, near=0.1, scale=1, cam_order=None):
    """The camera mosaic, uint8 [rows h, cols w, 3] on the frames' device (a CPU tensor for an array).  frames: uint8 [N, H, W,
    3]; boxes [n, >= 7]; colors uint8 [n, 3]; lidar2cam [N, 4, 4]; cam2img [N, 3 or 4, 3 or 4]; thickness in pixels (None: the
    reference's, default_camera_thickness(W)); cell i of the infer_grid(len(cam_order)) grid shows view cam_order[i]; scale = s
    writes the rounded mean (sum + s^2 // 2) // s^2 of each s x s block, h = H // s, w = W // s."""
    frames = _as_frames(frames)
    N, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    table = box_table(boxes)
    n, scale = table.shape[0], int(scale)
    if scale < 1:
        raise ValueError("scale must be an integer >= 1")
    pal, packed = _packed_colors(colors, n)
    L, K = as_lidar2cam(lidar2cam), as_cam2img(cam2img)
    if L.shape[0] != N or K.shape[0] != N:
        raise ValueError("%d frames, %d lidar2cam, %d cam2img" % (N, L.shape[0], K.shape[0]))
    order = list(range(N)) if cam_order is None else [int(c) for c in cam_order]
    if any(not 0 <= c < N for c in order):
        raise ValueError("cam_order names a view outside 0..%d" % (N - 1))
    rows, cols = infer_grid(len(order))
    cells = np.array(order + [-1] * (rows * cols - len(order)), np.int32)
    t = _thickness_units(thickness, default_camera_thickness(W))
    if not _frames_kernel_ok(frames, t, scale):
        PATHS["torch"] += 1
        return torch_composite(frames, camera_segments(table, L, K, near, t, H, W), pal, cells, rows, cols, scale)
    PATHS["kernel"] += 1
    dev = frames.device
    tab_d, L_d, K_d, col_d, cell_d = _upload(dev, table, L, K, packed, cells)
    nbytes = _lib.call_size("bfhip_vis_workspace_bytes", N, n, 12)
    work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.call("bfhip_vis_camera_segments", tab_d.data_ptr() if n else None, n, L_d.data_ptr(), K_d.data_ptr(), N, float(near),
                  t, H, W, work.data_ptr(), nbytes, _lib.stream_of(frames))
        return _kernel_composite(frames, work, nbytes, n, 12, col_d, cell_d, rows, cols, scale)


def bev_shape(xlim, ylim, px_per_m):
    return int(round((ylim[1] - ylim[0]) * px_per_m)), int(round((xlim[1] - xlim[0]) * px_per_m))


def render_bev(points, boxes, colors, xlim=(-50, 50), ylim=(-50, 50), px_per_m=10, point_size=1, thickness=None):
    """The bird's-eye plot, uint8 [H, W, 3] = bev_shape(...) on the points' device: black, every point of points [m, >= 2]
    with 0 <= floor((x - xlim0) px_per_m) < W (rows alike, counted from the top: matplotlib's y points up) a white point_size
    square, the footprints (corners 0, 3, 7, 4, 0) drawn over them.  thickness in pixels (None: DEFAULT_BEV_THICKNESS)."""
    if not torch.is_tensor(points):
        points = torch.from_numpy(np.ascontiguousarray(points))
    if points.dim() != 2 or points.shape[1] < 2:
        raise ValueError("points must be [m, 2 or more]")
    H, W = bev_shape(xlim, ylim, px_per_m)
    if not (1 <= H <= _MAX_DIM and 1 <= W <= _MAX_DIM):
        raise ValueError("a canvas of %d x %d pixels (1 .. %d a side)" % (H, W, _MAX_DIM))
    table = box_table(boxes)
    n, p = table.shape[0], int(point_size)
    if p < 1:
        raise ValueError("point_size must be an integer >= 1")
    pal, packed = _packed_colors(colors, n)
    t = _thickness_units(thickness, DEFAULT_BEV_THICKNESS)
    cells = np.zeros(1, np.int32)
    kernel = (ENABLED and points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and p <= 64
              and points.shape[0] < (1 << 31) and points.shape[1] <= 64)
    if not kernel:
        PATHS["torch"] += 1
        canvas = torch_bev_points(points, xlim[0], ylim[0], px_per_m, p, H, W)
        return torch_composite(canvas, bev_segments(table, xlim[0], ylim[1], px_per_m, t, H, W), pal, cells, 1, 1, 1)
    PATHS["kernel"] += 1
    dev = points.device
    tab_d, col_d, cell_d = _upload(dev, table, packed, cells)
    nbytes = _lib.call_size("bfhip_vis_workspace_bytes", 1, n, 4)
    work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    canvas = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev)
    m = int(points.shape[0])
    with torch.cuda.device(dev):
        stream = _lib.stream_of(points)
        _lib.call("bfhip_vis_bev_points", points.data_ptr() if m else None, m, int(points.shape[1]), float(xlim[0]), float(ylim[0]),
                  float(px_per_m), p, canvas.data_ptr(), H, W, stream)
        _lib.call("bfhip_vis_bev_segments", tab_d.data_ptr() if n else None, n, float(xlim[0]), float(ylim[1]), float(px_per_m), t,
                  H, W, work.data_ptr(), nbytes, stream)
        return _kernel_composite(canvas, work, nbytes, n, 4, col_d, cell_d, 1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- tracker
class Track:
    def __init__(self, det, track_id):
        self.det = np.array(det, copy=True)  # x, y, z, dx, dy, dz, yaw, score, label
        self.id = track_id
        self.missed = 0


class Tracker3D:
    """The reference tool's light tracker (visualize_bboxes_bevfusion.py:55-129): float32 centre distance in x, y, a cost of
    1e6 between classes, scipy's linear_sum_assignment, a pair kept when its cost is <= max_dist; an unmatched track ages and
    leaves once missed > max_missed; unmatched detections open tracks.  It never changes a box.  Host code: it decides which
    boxes are drawn."""

    def __init__(self, max_missed=3, max_dist=4.0):
        self.max_missed, self.max_dist = max_missed, max_dist
        self.tracks = []
        self.next_id = 1

    def _age(self, unmatched):
        for t in unmatched:
            t.missed += 1
        self.tracks = [t for t in self.tracks if t.missed <= self.max_missed]

    def _open(self, dets):
        for det in dets:
            self.tracks.append(Track(det, self.next_id))
            self.next_id += 1

    def update(self, detections):
        """detections [m, 9] (x, y, z, dx, dy, dz, yaw, score, label), or empty -> get_results()."""
        dets = np.asarray(detections)
        if dets.size == 0:
            self._age(self.tracks)
        elif not self.tracks:
            self._open(dets)
        else:
            from scipy.optimize import linear_sum_assignment
            cost = np.full((len(self.tracks), dets.shape[0]), 1e6, dtype=np.float32)
            for i, t in enumerate(self.tracks):
                for j, d in enumerate(dets):
                    if int(t.det[8]) == int(d[8]):
                        cost[i, j] = np.linalg.norm(t.det[:2] - d[:2])
            hit_t, hit_d = set(), set()
            for r, c in zip(*linear_sum_assignment(cost)):
                if cost[r, c] <= self.max_dist:
                    self.tracks[r].det = dets[c].copy()
                    self.tracks[r].missed = 0
                    hit_t.add(r)
                    hit_d.add(c)
            self._age([t for i, t in enumerate(self.tracks) if i not in hit_t])
            self._open([dets[j] for j in range(dets.shape[0]) if j not in hit_d])
        return self.get_results()

    def get_results(self):
        return [{"id": t.id, "box": t.det.copy()} for t in self.tracks]


# ----------------------------------------------------------------------------------------------------------------- sample
def _field(obj, name):
    if isinstance(obj, dict):
        if name in obj:
            return obj[name]
        return obj.get("metainfo", {}).get(name) if isinstance(obj.get("metainfo"), dict) else None
    return getattr(obj, name, None)


def select_boxes(pred_or_gt, score_thr=0.01, only=None, tracker=None):
    """(boxes float32 [n, 7], labels int64 [n]) to draw, as the reference's main loop picks them: predictions ({'bboxes_3d',
    'scores_3d', 'labels_3d'}, possibly under 'pred_instances_3d') are cut at score >= score_thr, filtered to the label indices
    `only`, and passed through `tracker` (its tracks are drawn); ground truth ({'gt_bboxes_3d', 'gt_labels_3d'}) is filtered
    only."""
    p = _field(pred_or_gt, "pred_instances_3d") or pred_or_gt
    if _field(p, "gt_bboxes_3d") is not None:
        boxes = _host(_field(p, "gt_bboxes_3d"), np.float32)
        boxes = boxes.reshape(-1, boxes.shape[-1] if boxes.size else 7)[:, :7]
        labels = _host(_field(p, "gt_labels_3d")).reshape(-1).astype(np.int64)
        if only is not None:
            keep = np.isin(labels, only)
            boxes, labels = boxes[keep], labels[keep]
        return boxes, labels
    boxes = _host(_field(p, "bboxes_3d"), np.float32)
    boxes = boxes.reshape(-1, boxes.shape[-1] if boxes.size else 7)[:, :7]
    labels = _field(p, "labels_3d")
    labels = np.zeros(len(boxes), np.int64) if labels is None else _host(labels).reshape(-1).astype(np.int64)
    scores = _field(p, "scores_3d")
    scores = np.ones(len(boxes), np.float32) if scores is None else _host(scores, np.float32).reshape(-1)
    keep = scores >= score_thr
    if only is not None:
        keep &= np.isin(labels, only)
    boxes, labels, scores = boxes[keep], labels[keep], scores[keep]
    if tracker is None:
        return boxes, labels
    dets = np.concatenate([boxes, scores[:, None], labels[:, None].astype(np.float32)], 1) if len(boxes) else np.zeros((0, 9), np.float32)
    tracked = tracker.update(dets)
    if not tracked:
        return np.zeros((0, 7), np.float32), np.zeros(0, np.int64)
    return (np.stack([t["box"][:7] for t in tracked]).astype(np.float32), np.array([int(t["box"][8]) for t in tracked], np.int64))


def visualize_sample(data_sample_or_meta, frames, points, pred_or_gt, classes, score_thr=0.01, only_classes=None, tracker=None,
                     cam_order=None, scale=1, near=0.1, thickness=None, xlim=(-50, 50), ylim=(-50, 50), px_per_m=10, point_size=1,
                     bev_thickness=None):
    """One sample as the reference's two tools show it -> (camera mosaic, BEV plot), both uint8 tensors.  The meta (a dict, or
    anything with the attributes) gives `ori_cam2img` and `lidar2cam`; frames: the uint8 [N, H, W, 3] block of jpeg.decode_frames
    (None: no mosaic); points [m, >= 2] (None: no BEV plot); only_classes: class names to keep."""
    only = None
    if only_classes:
        only = [classes.index(c) for c in only_classes if c in classes] or None
    boxes, labels = select_boxes(pred_or_gt, score_thr, only, tracker)
    colors = palette_colors(labels, classes)
    mosaic = bev = None
    if frames is not None:
        k, m = _field(data_sample_or_meta, "ori_cam2img"), _field(data_sample_or_meta, "lidar2cam")
        if k is None or m is None:
            raise ValueError("the sample carries no ori_cam2img / lidar2cam")
        mosaic = render_cameras(frames, boxes, colors, np.asarray(_host(m)), np.asarray(_host(k)), thickness=thickness, near=near,
                                scale=scale, cam_order=cam_order)
    if points is not None:
        bev = render_bev(points, boxes, colors, xlim=xlim, ylim=ylim, px_per_m=px_per_m, point_size=point_size,
                         thickness=bev_thickness)
    return mosaic, bev


@VISUALIZERS.register_module()
class PredictionVisualizer:
    """visualize_sample with its settings kept: `vis(meta, frames, points, pred_or_gt)` -> (mosaic, bev).  track=True keeps one
    Tracker3D across calls, as the reference's prediction loop does; **kwargs are visualize_sample's keywords."""

    def __init__(self, classes, score_thr=0.01, only_classes=None, track=True, max_missed=3, max_dist=4.0, **kwargs):
        self.classes, self.score_thr, self.only_classes, self.kwargs = list(classes), score_thr, only_classes, kwargs
        self.tracker = Tracker3D(max_missed=max_missed, max_dist=max_dist) if track else None

    def __call__(self, data_sample_or_meta, frames, points, pred_or_gt):
        return visualize_sample(data_sample_or_meta, frames, points, pred_or_gt, self.classes, score_thr=self.score_thr,
                                only_classes=self.only_classes, tracker=self.tracker, **self.kwargs)
