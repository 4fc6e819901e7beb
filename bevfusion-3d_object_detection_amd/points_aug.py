"""The LiDAR half of the reference's training pipeline, between loading and Pack3DDetInputs:

    BEVFusionGlobalRotScaleTrans (BF/transforms_3d.py:164-201) or GlobalRotScaleTrans (M3D/datasets/transforms/transforms_3d.py
    :631-808) -> BEVFusionRandomFlip3D (BF :130-161) -> PointsRangeFilter (M3D :904-956) -> ObjectRangeFilter (:844-901) ->
    ObjectNameFilter (:959-1001) -> PointShuffle (:811-841)

(the camera + LiDAR config has ImageAug3D in front of the chain and GridMask between ObjectNameFilter and PointShuffle: both are in
image_aug.py, and GridMask draws from np.random even when its prob is 0, so it belongs in the list for the same random stream)
under the reference's names, keywords and result keys, with the reference's np.random calls in the reference's order and its
float32 / float64 arithmetic for `pcd_rotation`, `lidar_aug_matrix` and the boxes (a few dozen rows: always on the host).
`points` is a float32 [n, C] tensor or array (C >= 3), `gt_bboxes_3d` a float32 [M, 7 or 9] tensor or array in LiDAR
convention with `gt_labels_3d` beside it; each comes back as the kind it came in.

The points' arithmetic is DEFINED here, by `torch_points_aug(points, plan)`, in elementwise float32 operations:

    x' = (x r00 + y r10) + z r20   (r = pcd_rotation = rot_mat_T; y' and z' likewise), every product and sum rounded once
    then (v + t) * s for R,T,S (the BEVFusion class) or v * s + t for R,S,T (the plain class)
    sign flips; the strict > min / < max test on the transformed xyz; order-preserving selection; the shuffle

The reference rotates with a matmul (or, without boxes, an einsum), whose bits depend on the BLAS path a shape takes (fused on
most rows, one ulp off the unfused order on about half of them); one order is fixed here instead and the tests hold it to the
reference within the rounding bound of a three-term dot product.

Three ways to the points:
  * `torch_points_aug(points, plan)`: plain torch on any device -- the specification, the fallback and the yardstick;
  * the transforms with defer=False: what the reference does, through `torch_points_aug` on the host, one step at a time;
    PointShuffle indexes by `torch.randperm(n)` exactly as the reference does;
  * defer=True (the four point transforms): the points are left untouched and each transform appends its step to
    `data["points_aug_plan"]` (PointsAugPlan); Det3DDataPreprocessor.process_points runs the plans of a batch on the device
    (`fused_points_aug`, csrc/points_aug.hip: count, scan, ranked write -- three launches and one host read of the kept counts).
    A plan holds at most one rotate / translate / scale group, then flips, then one range filter, then a shuffle, in that order.

ObjectSample (object_sample.py, in front of the chain in the LiDAR configs) adds a PASTE as the plan's first step: the sampled
objects' points `paste_points` [m, C] and their boxes as `paste_planes(boxes)` [K, 6, 4], six inward plane equations (normal, d)
per box by the reference's own sequence.  A point is inside a box when ((x n0 + y n1) + z n2) + d < 0 for all six planes, every
product and sum one float32 operation; the original points inside any box are dropped, the rows become [pasted points ;
surviving original points] and the rest of the plan runs on all of them.  On the device that is bfhip_points_aug_paste: at
most max_boxes() boxes per sample and pasted rows with the cloud's C, otherwise the torch path.

LoadPointsFromMultiSweeps (loading.py, the second step of the nuScenes configs) adds the SWEEP step in front of even that:
`points` is then [keyframe ; sweep 1 ; ... ; sweep S] as read from the files, `sweep_starts` the S + 2 row boundaries.  A sweep
row is dropped when |x| < radius and |y| < radius (raw float32; a NaN keeps the row), its xyz become
float32((double(x) m0j + double(y) m1j) + double(z) m2j), then float32(double(v_j) - t_j), with m, t of the float64
`lidar2sensor` -- the reference's `p[:, :3] @ m` and `-= t`, every product and sum one float64 operation -- and column 4 becomes
the sweep's float32 time lag (0 on the keyframe).  The box test of a paste runs on these xyz.  On the device that is
bfhip_points_aug_sweeps: at most max_sweeps() segments (keyframe included) and C >= 5, otherwise the torch path.

The deferred shuffle departs from the reference on purpose: `randperm(n)` needs n, which exists only after the filter ran on
the device.  PointShuffle(defer=True) draws one 64-bit seed with `torch.randint` from torch's global generator instead and the
order is `shuffle_permutation(seed, n_kept)`: a keyed Feistel network on the next even power of two with cycle walking, integer
operations only, the same in torch and in the kernel.

BFHIP_POINTS_AUG (ships on; measured with tools/points_aug_micro.py: DESIGN.md section 6): 0 sends every deferred batch through
`torch_points_aug`.  CPU tensors, other dtypes and non-contiguous points go that way as well, with the same bits.  PATHS counts
the deferred batches each way took.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .registry import TRANSFORMS

ENABLED = os.environ.get("BFHIP_POINTS_AUG", "1") != "0"
PATHS = {"kernel": 0, "torch": 0}  # deferred point batches taken by each path (tests, tools)

ROUNDS = 6  # BFHIP_POINTS_AUG_ROUNDS
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
_STAGES = {"rts": 1, "flip": 2, "range": 3, "shuffle": 4}


class PointsAugPlan:
    """What the deferred point transforms of ONE sample add up to; small, picklable, left on the host by
    Det3DDataPreprocessor.cast_data.  rot float32 [3, 3] (rot_mat_T), trans float32 [3], scale float32, order "RTS" / "RST" (None:
    no such step), flip_horizontal (y) / flip_vertical (x), range float32 [6] or None, shuffle + its 64-bit seed.  ObjectSample's
    paste, the step in front of all of these: paste_points float32 [m, C] and paste_planes float32 [K, 6, 4], both None
    without one (such a plan's pickled state holds neither).  LoadPointsFromMultiSweeps' sweep step, in front of the paste:
    sweep_starts int64 [S + 2] (row boundaries of keyframe and sweeps), sweep_l2s float64 [S, 4, 4] or None (no transform),
    sweep_dt float32 [S], sweep_remove, sweep_radius float32; all None without one (and absent from the pickled state)."""
    __slots__ = ("rot", "trans", "scale", "order", "flip_horizontal", "flip_vertical", "range", "shuffle", "seed", "stage",
                 "paste_points", "paste_planes", "sweep_starts", "sweep_l2s", "sweep_dt", "sweep_remove", "sweep_radius")
    _PASTE = ("paste_points", "paste_planes")
    _SWEEPS = ("sweep_starts", "sweep_l2s", "sweep_dt", "sweep_remove", "sweep_radius")

    def __init__(self):
        self.paste_points = self.paste_planes = None
        self.sweep_starts = self.sweep_l2s = self.sweep_dt = self.sweep_remove = self.sweep_radius = None
        self.rot = np.eye(3, dtype=np.float32)
        self.trans = np.zeros(3, np.float32)
        self.scale = np.float32(1.0)
        self.order = None
        self.flip_horizontal = self.flip_vertical = False
        self.range = None
        self.shuffle = False
        self.seed = 0
        self.stage = 0

    def __getstate__(self):
        return {k: getattr(self, k) for k in self.__slots__
                if (k not in self._PASTE or self.paste_points is not None) and (k not in self._SWEEPS or self.sweep_starts is not None)}

    def __setstate__(self, state):
        self.paste_points = self.paste_planes = None
        self.sweep_starts = self.sweep_l2s = self.sweep_dt = self.sweep_remove = self.sweep_radius = None
        for k, v in state.items():
            setattr(self, k, v)

    def _enter(self, step):
        if _STAGES[step] <= self.stage:
            raise ValueError("points_aug_plan: a %s step cannot follow what the plan already holds (one rotate / translate / scale "
                             "group, then flips, then one range filter, then a shuffle); run this pipeline with defer=False" % step)
        self.stage = _STAGES[step]

    def set_sweeps(self, starts, lidar2sensor, dt, remove_close, radius=1.0):
        """LoadPointsFromMultiSweeps' step: the points are [keyframe ; sweep 1 ; ... ; sweep S] and starts [S + 2] their row
        boundaries (0, the keyframe's rows, ..., all rows).  lidar2sensor float64 [S, 4, 4] (None: the sweeps are not
        transformed -- the padded copies of a keyframe), dt [S] the sweeps' float32 time lags.  The very first step of a plan,
        once; it does not advance `stage`, so a paste may follow."""
        if self.stage != 0 or self.paste_points is not None or self.sweep_starts is not None:
            raise ValueError("points_aug_plan: the sweep step must be the first step of a plan, and there is one per plan; run this "
                             "pipeline with defer=False")
        starts = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).reshape(-1))
        dt = np.ascontiguousarray(np.asarray(dt, dtype=np.float32).reshape(-1))
        S = len(dt)
        if len(starts) != S + 2 or starts[0] != 0 or (np.diff(starts) < 0).any():
            raise ValueError("set_sweeps: starts must be %d non-decreasing row boundaries from 0, got %s" % (S + 2, starts.tolist()))
        if lidar2sensor is not None:
            lidar2sensor = np.ascontiguousarray(np.asarray(lidar2sensor, dtype=np.float64).reshape(-1, 4, 4))
            if len(lidar2sensor) != S:
                raise ValueError("set_sweeps: %d lidar2sensor matrices for %d sweeps" % (len(lidar2sensor), S))
        self.sweep_starts, self.sweep_l2s, self.sweep_dt = starts, lidar2sensor, dt
        self.sweep_remove, self.sweep_radius = bool(remove_close), np.float32(radius)
        return self

    def set_paste(self, points, boxes):
        """ObjectSample's paste: points float32 [m, C], the sampled objects' points at their boxes; boxes [K, 7+], the sampled
        boxes.  The original points inside any of them are dropped and `points` go in front of the rest.  First step only (a
        sweep step may stand in front of it)."""
        if self.stage != 0 or self.paste_points is not None:
            raise ValueError("points_aug_plan: a paste must be the first step of a plan, and there is one per plan; run this "
                             "pipeline with defer=False")
        points = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
        if points.ndim != 2 or points.shape[1] < 3:
            raise ValueError("set_paste: points must be [m, C] with C >= 3, got %s" % (points.shape,))
        self.paste_points, self.paste_planes = points, paste_planes(boxes)
        return self

    def set_rts(self, rot, trans, scale, order):
        if order not in ("RTS", "RST"):
            raise ValueError("order must be 'RTS' or 'RST', got %r" % (order,))
        self._enter("rts")
        self.rot = np.ascontiguousarray(np.asarray(rot, dtype=np.float32).reshape(3, 3))
        self.trans = np.ascontiguousarray(np.asarray(trans, dtype=np.float32).reshape(3))
        self.scale = np.float32(scale)
        self.order = order
        return self

    def set_flip(self, horizontal, vertical):
        self._enter("flip")
        self.flip_horizontal, self.flip_vertical = bool(horizontal), bool(vertical)
        return self

    def set_range(self, point_cloud_range):
        self._enter("range")
        self.range = np.ascontiguousarray(np.asarray(point_cloud_range, dtype=np.float32).reshape(6))
        return self

    def set_shuffle(self, seed):
        self._enter("shuffle")
        self.shuffle, self.seed = True, int(seed) & _M64
        return self

    def flags(self):
        """The `flags` of bfhip_points_aug_sample."""
        return ((1 if self.order is not None else 0) | (2 if self.order == "RST" else 0) | (4 if self.flip_horizontal else 0) |
                (8 if self.flip_vertical else 0) | (16 if self.range is not None else 0) | (32 if self.shuffle else 0))


# ---------------------------------------------------------------------------------------------- the shuffle
def shuffle_keys(seed):
    """The ROUNDS 32-bit round keys of a 64-bit seed: the low halves of consecutive splitmix64 outputs."""
    z, keys = int(seed) & _M64, []
    for _ in range(ROUNDS):
        z = (z + 0x9E3779B97F4A7C15) & _M64
        x = z
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
        x ^= x >> 31
        keys.append(x & _M32)
    return keys


def _mix32(x):
    """int64 tensor holding 32-bit values: the kernel's mix32 (products stay below 2^59, so int64 never wraps)."""
    x = (((x >> 16) ^ x) * 0x45D9F3B) & _M32
    x = (((x >> 16) ^ x) * 0x45D9F3B) & _M32
    return (x >> 16) ^ x


def shuffle_permutation(seed, n, device=None):
    """int64 [n]: perm[r] = the output row of the r-th kept point; a bijection of [0, n).  A balanced Feistel network of ROUNDS
    rounds on 2 h bits, h = max(1, ceil(bitlength(n - 1) / 2)), round i: (L, R) <- (R, L ^ (mix32(R + key_i) & (2^h - 1))),
    re-applied while the value is >= n.  The network is a bijection of [0, 4^h) whatever the round function, so the walk
    follows the cycle of r and comes back into [0, n): it terminates, and distinct r end on distinct rows."""
    return shuffle_permutations([seed], n, device)[0]


def shuffle_permutations(seeds, n, device=None):
    """int64 [len(seeds), n]: shuffle_permutation of every seed at once."""
    n = int(n)
    v = torch.arange(n, dtype=torch.int64, device=device).repeat(len(seeds), 1)
    if n == 0:
        return v
    h = max(1, ((n - 1).bit_length() + 1) // 2)
    mask = (1 << h) - 1
    keys = torch.tensor([shuffle_keys(s) for s in seeds], dtype=torch.int64, device=device)

    def network(v):
        L, R = v >> h, v & mask
        for i in range(ROUNDS):
            L, R = R, L ^ (_mix32((R + keys[:, i:i + 1]) & _M32) & mask)
        return (L << h) | R

    out = network(v)
    while True:
        bad = out >= n
        if not bool(bad.any()):
            return out
        out = torch.where(bad, network(out), out)


# ---------------------------------------------------------------------------------------------- the defined arithmetic
def _as_points(points):
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(np.ascontiguousarray(points))
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] < 3:
        raise ValueError("points must be a [n, C] tensor or array with C >= 3")
    return points if points.dtype == torch.float32 else points.to(torch.float32)


def _range_mask(x, y, z, rng):
    lo0, lo1, lo2, hi0, hi1, hi2 = (float(v) for v in rng)
    return (x > lo0) & (y > lo1) & (z > lo2) & (x < hi0) & (y < hi1) & (z < hi2)


def transformed_xyz(points, plan):
    """(x, y, z) float32 [n] each: the plan's rotate / translate / scale and flips of points[:, :3]."""
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    if plan.order is not None:
        r = [[float(v) for v in row] for row in plan.rot]
        t = [float(v) for v in plan.trans]
        s = float(plan.scale)
        x, y, z = ((x * r[0][0] + y * r[1][0]) + z * r[2][0],
                   (x * r[0][1] + y * r[1][1]) + z * r[2][1],
                   (x * r[0][2] + y * r[1][2]) + z * r[2][2])
        if plan.order == "RTS":
            x, y, z = (x + t[0]) * s, (y + t[1]) * s, (z + t[2]) * s
        else:
            x, y, z = x * s + t[0], y * s + t[1], z * s + t[2]
    if plan.flip_horizontal:
        y = -y
    if plan.flip_vertical:
        x = -x
    return x, y, z


def _rotate_z(corners, angles):
    """rotation_3d_in_axis(corners [K, P, 2 or 3], angles [K], axis=2) as the reference's numpy callers reach it: through float32
    torch tensors and the 'aij,jka->aik' einsum (M3D/structures/bbox_3d/utils.py:20-124), back in the corners' dtype."""
    pts = torch.tensor(corners, dtype=torch.float32)
    ang = torch.tensor(angles, dtype=torch.float32)
    rot_sin, rot_cos = torch.sin(ang), torch.cos(ang)
    if pts.shape[-1] == 3:
        ones, zeros = torch.ones_like(rot_cos), torch.zeros_like(rot_cos)
        rot = torch.stack([torch.stack([rot_cos, rot_sin, zeros]), torch.stack([-rot_sin, rot_cos, zeros]),
                           torch.stack([zeros, zeros, ones])])
    else:
        rot = torch.stack([torch.stack([rot_cos, rot_sin]), torch.stack([-rot_sin, rot_cos])])
    out = torch.einsum("aij,jka->aik", pts, rot) if pts.shape[0] else pts
    return out.numpy().astype(corners.dtype)


def box_corners(centers, dims, angles, origin):
    """center_to_corner_box2d / center_to_corner_box3d(axis=2) (M3D/structures/ops/box_np_ops.py:63-201): [K, 4, 2] clockwise
    from the minimum corner, or [K, 8, 3]; in the boxes' dtype."""
    ndim = int(dims.shape[1])
    norm = np.stack(np.unravel_index(np.arange(2 ** ndim), [2] * ndim), axis=1).astype(dims.dtype)
    norm = norm[[0, 1, 3, 2]] if ndim == 2 else norm[[0, 1, 3, 2, 4, 5, 7, 6]]
    norm = norm - np.array(origin, dtype=dims.dtype)
    corners = dims.reshape([-1, 1, ndim]) * norm.reshape([1, 2 ** ndim, ndim])
    corners = _rotate_z(corners, angles)
    corners += centers.reshape([-1, 1, ndim])
    return corners


_SURFACES = ((0, 1, 2, 3), (7, 6, 5, 4), (0, 3, 7, 4), (1, 5, 6, 2), (0, 4, 5, 1), (3, 2, 6, 7))  # corner_to_surfaces_3d


def paste_planes(boxes):
    """boxes [K, 7+] (x, y, z of the bottom centre, dx, dy, dz, yaw) -> float32 [K, 6, 4]: per box the six inward plane
    equations (n0, n1, n2, d), by the sequence points_in_rbbox takes (box_np_ops.py:354-377): center_to_corner_box3d(origin=(0.5,
    0.5, 0), axis=2) -> corner_to_surfaces_3d -> surface_equ_3d, in the boxes' arithmetic (float32 for float32 boxes)."""
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or boxes.shape[1] < 7:
        raise ValueError("boxes must be [K, 7 or more], got %s" % (boxes.shape,))
    if not np.issubdtype(boxes.dtype, np.floating):
        boxes = boxes.astype(np.float32)
    if boxes.shape[0] == 0:
        return np.zeros((0, 6, 4), np.float32)
    corners = box_corners(boxes[:, :3], boxes[:, 3:6], boxes[:, 6], (0.5, 0.5, 0))
    surfaces = np.array([[corners[:, i] for i in face] for face in _SURFACES]).transpose([2, 0, 1, 3])[:, :, :3, :]  # [K, 6, 3, 3]
    vec = surfaces[:, :, :2, :] - surfaces[:, :, 1:3, :]
    normal = np.cross(vec[:, :, 0, :], vec[:, :, 1, :])
    d = -np.einsum("aij, aij->ai", normal, surfaces[:, :, 0, :])
    return np.ascontiguousarray(np.concatenate([normal, d[:, :, None]], 2).astype(np.float32))


def points_in_any_box(points, planes):
    """bool [n]: the rows of `points` (float32 [n, C] tensor) inside any box of `planes` (float32 [K, 6, 4] tensor on the same
    device): for all six planes ((x n0 + y n1) + z n2) + d < 0, every product and sum one float32 operation."""
    n = int(points.shape[0])
    xyz = points[:, :3].t().contiguous()  # [3, n]: the pairs as [K, n], points along the contiguous axis
    step = 16384 if points.device.type == "cpu" else max(n, 1)  # on the host: temporaries that stay in the cache
    pairs = []
    for s in range(0, n, step):  # two opposite faces, every (box, point) pair: a slab per box, which few pairs are in
        x, y, z = xyz[0:1, s:s + step], xyz[1:2, s:s + step], xyz[2:3, s:s + step]
        pl = planes[:, 0, :, None]
        inside = (((x * pl[:, 0] + y * pl[:, 1]) + z * pl[:, 2]) + pl[:, 3]) < 0
        pl = planes[:, 1, :, None]
        inside &= (((x * pl[:, 0] + y * pl[:, 1]) + z * pl[:, 2]) + pl[:, 3]) < 0
        b, p = torch.nonzero(inside, as_tuple=True)
        pairs.append((b, p + s))
    bi = torch.cat([b for b, _ in pairs]) if pairs else torch.zeros(0, dtype=torch.int64, device=points.device)
    pi = torch.cat([p for _, p in pairs]) if pairs else bi
    x, y, z = points[pi, 0], points[pi, 1], points[pi, 2]
    for k in range(2, 6):  # the other four faces for those pairs only: the same operations on the same operands
        pl = planes[bi, k, :]
        keep = (((x * pl[:, 0] + y * pl[:, 1]) + z * pl[:, 2]) + pl[:, 3]) < 0
        pi, bi, x, y, z = pi[keep], bi[keep], x[keep], y[keep], z[keep]
    out = torch.zeros(points.shape[0], dtype=torch.bool, device=points.device)
    out[pi] = True
    return out


def sweep_rows(p, plan):
    """The sweep step of a plan on p = [keyframe ; sweep 1 ; ... ; sweep S] (float32 [n, C] tensor, C >= 5): the rows that are
    left, sweeps through lidar2sensor, column 4 the time lag.  The arithmetic of the module docstring."""
    starts = [int(v) for v in plan.sweep_starts]
    if p.shape[1] < 5 or starts[-1] != p.shape[0]:
        raise ValueError("points_aug_plan: the sweep step needs [n, C >= 5] points with n = %d rows, got %s"
                         % (starts[-1], tuple(p.shape)))
    radius = float(plan.sweep_radius)
    key = p[:starts[1]].clone()
    key[:, 4] = 0
    parts = [key]
    for i in range(len(starts) - 2):
        q = p[starts[i + 1]:starts[i + 2]]
        if plan.sweep_remove:
            q = q[~((q[:, 0].abs() < radius) & (q[:, 1].abs() < radius))]
        q = q.clone()
        if plan.sweep_l2s is not None:
            m = [[float(v) for v in row] for row in plan.sweep_l2s[i]]
            x, y, z = q[:, 0].double(), q[:, 1].double(), q[:, 2].double()
            for j in range(3):
                v = ((x * m[0][j] + y * m[1][j]) + z * m[2][j]).float()
                q[:, j] = (v.double() - m[j][3]).float()
        q[:, 4] = float(plan.sweep_dt[i])
        parts.append(q)
    return torch.cat(parts, 0)


def torch_points_aug(points, plan, return_mask=False):
    """points [n, C] (tensor on any device, or array) + PointsAugPlan -> float32 [kept, C] on the points' device: the
    specification csrc/points_aug.hip restates bit for bit.  return_mask: also the bool of the rows the filter kept (with a
    paste or a sweep step: of the rows [pasted points ; surviving original points], which the rest of the plan runs on)."""
    p = _as_points(points)
    if plan.sweep_starts is not None:
        p = sweep_rows(p, plan)
    if plan.paste_points is not None:
        pasted = torch.from_numpy(plan.paste_points).to(p.device)
        if pasted.shape[1] != p.shape[1]:
            raise ValueError("points_aug_plan: pasted points have %d columns, the cloud has %d" % (pasted.shape[1], p.shape[1]))
        inside = points_in_any_box(p, torch.from_numpy(plan.paste_planes).to(p.device))
        p = torch.cat([pasted, p[~inside]], 0)
    x, y, z = transformed_xyz(p, plan)
    out = torch.cat([torch.stack([x, y, z], 1), p[:, 3:]], 1)
    mask = None
    if plan.range is not None:
        mask = _range_mask(x, y, z, plan.range)
        out = out[mask]
    elif return_mask:
        mask = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
    if plan.shuffle:
        perm = shuffle_permutation(plan.seed, out.shape[0], out.device)
        dst = torch.empty_like(out)
        dst[perm] = out
        out = dst
    return (out, mask) if return_mask else out


# ---------------------------------------------------------------------------------------------- the device path
class _Sample(ctypes.Structure):
    """bfhip_points_aug_sample (include/bevfusion_hip.h)."""
    _fields_ = [("points", ctypes.c_void_p), ("n", ctypes.c_int), ("flags", ctypes.c_int), ("rot", ctypes.c_float * 9),
                ("trans", ctypes.c_float * 3), ("scale", ctypes.c_float), ("range", ctypes.c_float * 6),
                ("keys", ctypes.c_uint32 * ROUNDS)]


class _Paste(ctypes.Structure):
    """bfhip_points_aug_paste_desc (include/bevfusion_hip.h)."""
    _fields_ = [("points", ctypes.c_void_p), ("n_points", ctypes.c_int), ("planes", ctypes.c_void_p), ("n_boxes", ctypes.c_int)]


class _Sweeps(ctypes.Structure):
    """bfhip_points_aug_sweeps_desc (include/bevfusion_hip.h)."""
    _fields_ = [("segments", ctypes.c_void_p), ("n_segments", ctypes.c_int), ("first", ctypes.c_int * 17)]


# bfhip_points_aug_segment: 112 bytes, the doubles 8-byte aligned
SEGMENT = np.dtype([("first", "<i4"), ("flags", "<i4"), ("dt", "<f4"), ("radius", "<f4"), ("m", "<f8", (9,)), ("t", "<f8", (3,))])


def max_sweeps():
    """The most segments per sample, keyframe included, the kernels take (bfhip_points_aug_max_sweeps)."""
    return int(_lib.load().bfhip_points_aug_max_sweeps())


def sweep_segments(plan):
    """The plan's segment table, SEGMENT [S + 1]: the keyframe (flags 0, dt 0), then per sweep flags 1 (remove close) | 2
    (transform), its dt, the 3 x 3 of lidar2sensor row-major and its translation column."""
    S = len(plan.sweep_dt)
    seg = np.zeros(S + 1, SEGMENT)
    seg["first"] = plan.sweep_starts[:-1]
    seg["radius"] = plan.sweep_radius
    seg["flags"][1:] = (1 if plan.sweep_remove else 0) | (2 if plan.sweep_l2s is not None else 0)
    seg["dt"][1:] = plan.sweep_dt
    if plan.sweep_l2s is not None:
        seg["m"][1:] = plan.sweep_l2s[:, :3, :3].reshape(S, 9)
        seg["t"][1:] = plan.sweep_l2s[:, :3, 3]
    return seg


def max_boxes():
    """The most pasted boxes per sample the kernels take (bfhip_points_aug_max_boxes)."""
    return int(_lib.load().bfhip_points_aug_max_boxes())


def fused_supported(points, plans=()):
    """True when bfhip_points_aug / bfhip_points_aug_paste / bfhip_points_aug_sweeps takes this batch: float32 contiguous [n, C]
    device tensors on one device, one C in 3 .. 8, fewer than 2^31 rows in all (pasted ones included); every paste with the
    cloud's C and at most max_boxes() boxes; every sweep step with at most max_sweeps() segments, its rows the sample's, C >= 5."""
    if not points or not all(torch.is_tensor(p) and p.is_cuda and p.dtype == torch.float32 and p.dim() == 2
                             and p.is_contiguous() and p.device == points[0].device and p.shape[1] == points[0].shape[1]
                             for p in points):
        return False
    pastes = [plan for plan in plans if plan.paste_points is not None]
    if pastes and not all(plan.paste_points.shape[1] == points[0].shape[1] and plan.paste_planes.shape[0] <= max_boxes()
                          for plan in pastes):
        return False
    swept = [(p, plan) for p, plan in zip(points, plans) if plan.sweep_starts is not None]
    if swept and not (points[0].shape[1] >= 5 and all(len(plan.sweep_starts) - 1 <= max_sweeps() and
                                                      int(plan.sweep_starts[-1]) == p.shape[0] for p, plan in swept)):
        return False
    rows = sum(int(p.shape[0]) for p in points) + sum(int(plan.paste_points.shape[0]) for plan in pastes)
    return 3 <= points[0].shape[1] <= 8 and rows < (1 << 31)


def descriptors(points, plans):
    """The bfhip_points_aug_sample array of a batch."""
    descs = (_Sample * len(points))()
    for d, p, plan in zip(descs, points, plans):
        d.points, d.n, d.flags = (p.data_ptr() if p.shape[0] else None), int(p.shape[0]), plan.flags()
        d.rot[:] = [float(v) for v in plan.rot.reshape(-1)]
        d.trans[:] = [float(v) for v in plan.trans]
        d.scale = float(plan.scale)
        d.range[:] = [float(v) for v in plan.range] if plan.range is not None else [0.0] * 6
        d.keys[:] = shuffle_keys(plan.seed) if plan.shuffle else [0] * ROUNDS
    return descs


def table_descriptors(plans, dev):
    """(the bfhip_points_aug_paste_desc array or None when no plan has a paste, the bfhip_points_aug_sweeps_desc array or None
    when no plan has a sweep step, the device tensor both point into): the plans' segment tables, then every plan's pasted rows
    and plane table, packed into ONE pinned host buffer and uploaded with ONE non-blocking copy on the current stream."""
    tables = [sweep_segments(plan) if plan.sweep_starts is not None else None for plan in plans]
    pasted = [plan for plan in plans if plan.paste_points is not None]
    parts = [t.view(np.uint8) for t in tables if t is not None]
    parts += [a.reshape(-1).view(np.uint8) for plan in pasted for a in (plan.paste_points, plan.paste_planes)]
    host = torch.empty(sum(a.size for a in parts), dtype=torch.uint8, pin_memory=True)
    if host.numel():
        np.concatenate(parts, out=host.numpy())
    table = torch.empty(host.numel(), dtype=torch.uint8, device=dev)  # the allocator's blocks are 512-byte aligned
    table.copy_(host, non_blocking=True)
    at, base = 0, table.data_ptr()  # byte offsets; a zero-initialised descriptor is an empty one
    sweeps = (_Sweeps * len(plans))() if any(t is not None for t in tables) else None
    for i, t in enumerate(tables):
        if t is not None:
            d = sweeps[i]
            d.segments, d.n_segments = base + at, len(t)  # 112-byte entries in front, from an aligned base: 8-byte aligned
            d.first[:len(t) + 1] = [int(v) for v in plans[i].sweep_starts]
            at += t.nbytes
    pastes = (_Paste * len(plans))() if pasted else None
    for i, plan in enumerate(plans):
        if plan.paste_points is not None:
            d, m, k = pastes[i], plan.paste_points.shape[0], plan.paste_planes.shape[0]
            d.points, d.n_points = (base + at if m else None), m
            at += plan.paste_points.nbytes
            d.planes, d.n_boxes = (base + at if k else None), k
            at += plan.paste_planes.nbytes
    return pastes, sweeps, table


def fused_points_aug(points, plans):
    """points: list of device float32 [n_i, C]; plans: list of PointsAugPlan -> the list of [kept_i, C] tensors, views of one
    buffer of sum(n_i + pasted rows of i) rows.  Three launches per 16 samples, then ONE host read per batch: the B kept counts,
    which the views' shapes need (it waits for the launches).  Plans with a paste or a sweep step add one host-to-device copy per
    batch (table_descriptors): a batch in which any plan has a sweep step goes through bfhip_points_aug_sweeps, otherwise one
    with a paste through bfhip_points_aug_paste, and a batch with neither takes bfhip_points_aug, with no upload at all."""
    B, C, dev = len(points), int(points[0].shape[1]), points[0].device
    sizes = [int(p.shape[0]) + (len(plan.paste_points) if plan.paste_points is not None else 0) for p, plan in zip(points, plans)]
    total = sum(sizes)
    out = torch.empty((total, C), dtype=torch.float32, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = _lib.call_size("bfhip_points_aug_workspace_bytes", total, B)
    work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    descs = descriptors(points, plans)
    tail = (B, C, out.data_ptr() if total else None, kept.data_ptr(), work.data_ptr(), nbytes, _lib.stream_of(out))
    with torch.cuda.device(dev):
        if any(plan.paste_points is not None or plan.sweep_starts is not None for plan in plans):
            pastes, sweeps, table = table_descriptors(plans, dev)  # `table` owns the device memory the descriptors point into
            if sweeps is not None:
                _lib.call("bfhip_points_aug_sweeps", descs, pastes, sweeps, *tail)
            else:
                _lib.call("bfhip_points_aug_paste", descs, pastes, *tail)
        else:
            _lib.call("bfhip_points_aug", descs, *tail)
    counts = kept.cpu().tolist()  # the batch's one host read
    views, row = [], 0
    for n, k in zip(sizes, counts):
        views.append(out[row:row + k])
        row += n
    return views


def process_points(points, plans):
    """Deferred point transforms of a batch: points = per sample [n_i, C], plans = per sample the PointsAugPlan -> the list of
    float32 [kept_i, C] tensors (views of one buffer), the bits of [torch_points_aug(p, plan) ...].  On the GPU through
    csrc/points_aug.hip, which costs one host read per batch (the kept counts)."""
    points = list(points)
    plans = [plans] if isinstance(plans, PointsAugPlan) else list(plans)
    if len(points) != len(plans) or not points:
        raise ValueError("points_aug_plan: %d plans for %d samples" % (len(plans), len(points)))
    if not all(isinstance(p, PointsAugPlan) for p in plans):
        raise TypeError("points_aug_plan: every sample needs a PointsAugPlan")
    if ENABLED and fused_supported(points, plans):
        PATHS["kernel"] += 1
        return fused_points_aug(points, plans)
    PATHS["torch"] += 1
    outs = [torch_points_aug(p, plan) for p, plan in zip(points, plans)]
    if len({o.shape[1] for o in outs}) != 1 or len({o.device for o in outs}) != 1:
        return outs
    return list(torch.cat(outs, 0).split([int(o.shape[0]) for o in outs], 0))


# ---------------------------------------------------------------------------------------------- the transforms
def _unwrap(value):
    """(float32 tensor that may be edited in place, was it an array)."""
    if isinstance(value, np.ndarray):
        return torch.from_numpy(np.array(value, dtype=np.float32)), True
    return torch.as_tensor(value).to(torch.float32).clone(), False


def _wrap(tensor, was_array):
    return tensor.numpy() if was_array else tensor


def _plan_of(data):
    for key in ("pts_instance_mask", "pts_semantic_mask"):
        if data.get(key) is not None:
            raise ValueError("defer=True does not carry %s through the filter and the shuffle; use defer=False" % key)
    plan = data.get("points_aug_plan")
    if plan is None:
        plan = data["points_aug_plan"] = PointsAugPlan()
    return plan


def _apply(data, plan):
    """One eager step on data["points"]; the filter's mask, if any."""
    pts = data["points"]
    out, mask = torch_points_aug(pts, plan, return_mask=True)
    data["points"] = out.numpy() if isinstance(pts, np.ndarray) else out
    return mask


def rotation_matrix(angle):
    """(rot_mat_T float32 [3, 3], the float32 angle): rotation_3d_in_axis(..., axis=2, return_mat=True) of one angle, operation
    for operation (M3D/structures/bbox_3d/utils.py:64-121)."""
    angle = torch.tensor(angle, dtype=torch.float32)
    angles = torch.full((1,), angle)
    rot_sin, rot_cos = torch.sin(angles), torch.cos(angles)
    ones, zeros = torch.ones_like(rot_cos), torch.zeros_like(rot_cos)
    rot = torch.stack([torch.stack([rot_cos, rot_sin, zeros]), torch.stack([-rot_sin, rot_cos, zeros]),
                       torch.stack([zeros, zeros, ones])])
    return torch.einsum("jka->ajk", rot).squeeze(0), angle


@TRANSFORMS.register_module()
class GlobalRotScaleTrans:
    """The reference's GlobalRotScaleTrans: rotate about z, scale, translate (`transformation_3d_flow` gets R, S, T).  Writes
    pcd_rotation (float32 tensor [3, 3], rot_mat_T), pcd_rotation_angle, pcd_scale_factor, pcd_trans."""
    ORDER = "RST"

    def __init__(self, rot_range=(-0.78539816, 0.78539816), scale_ratio_range=(0.95, 1.05), translation_std=(0, 0, 0),
                 shift_height=False, defer=False):
        seq = (list, tuple, np.ndarray)
        if not isinstance(rot_range, seq):
            rot_range = [-rot_range, rot_range]
        if not isinstance(scale_ratio_range, seq):
            raise TypeError("unsupported scale_ratio_range type %s" % type(scale_ratio_range))
        if not isinstance(translation_std, seq):
            translation_std = [translation_std] * 3
        if not all(std >= 0 for std in translation_std):
            raise ValueError("translation_std should be positive")
        if defer and shift_height:
            raise ValueError("defer=True does not scale a height column (shift_height=True); use defer=False")
        self.rot_range, self.scale_ratio_range, self.translation_std = rot_range, scale_ratio_range, translation_std
        self.shift_height, self.defer = bool(shift_height), bool(defer)

    def transform(self, data):
        if "transformation_3d_flow" not in data:
            data["transformation_3d_flow"] = []
        noise_rotation = np.random.uniform(self.rot_range[0], self.rot_range[1])
        if "pcd_scale_factor" not in data:
            data["pcd_scale_factor"] = np.random.uniform(self.scale_ratio_range[0], self.scale_ratio_range[1])
        trans = np.random.normal(scale=np.array(self.translation_std, dtype=np.float32), size=3).T
        scale = data["pcd_scale_factor"]
        rot, angle = rotation_matrix(noise_rotation)
        data["pcd_rotation"], data["pcd_rotation_angle"], data["pcd_trans"] = rot, noise_rotation, trans

        if "gt_bboxes_3d" in data:
            b, was_array = _unwrap(data["gt_bboxes_3d"])
            if len(b):  # LiDARInstance3DBoxes.rotate
                b[:, 0:3] = torch.einsum("aij,jka->aik", b[:, 0:3][None], rot[:, :, None]).squeeze(0)
                b[:, 6] += angle
                if b.shape[1] == 9:
                    b[:, 7:9] = b[:, 7:9] @ rot[:2, :2]
            steps = {"T": lambda: b[:, :3].add_(b.new_tensor(trans)),
                     "S": lambda: (b[:, :6].mul_(scale), b[:, 7:].mul_(scale)) if len(b) else None}
            for step in self.ORDER[1:]:
                steps[step]()
            data["gt_bboxes_3d"] = _wrap(b, was_array)

        if self.defer:
            _plan_of(data).set_rts(rot.numpy(), trans, scale, self.ORDER)
        else:
            _apply(data, PointsAugPlan().set_rts(rot.numpy(), trans, scale, self.ORDER))
            if self.shift_height:  # the reference scales the height attribute too; its column is the caller's to name
                col = data.get("points_height_dim")
                if col is None:
                    raise ValueError("shift_height=True needs data['points_height_dim'], the column of the height attribute")
                pts = data["points"]
                pts[:, col] = pts[:, col] * np.float32(scale)
        data["transformation_3d_flow"].extend(list(self.ORDER))
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class BEVFusionGlobalRotScaleTrans(GlobalRotScaleTrans):
    """The BEVFusion configs' variant: rotate, translate, scale (R, T, S), and the 4 x 4 float64 `lidar_aug_matrix` the view
    transform consumes."""
    ORDER = "RTS"

    def transform(self, data):
        data = super().transform(data)
        lidar_augs = np.eye(4)
        lidar_augs[:3, :3] = (data["pcd_rotation"].T * data["pcd_scale_factor"]).numpy()
        lidar_augs[:3, 3] = data["pcd_trans"] * data["pcd_scale_factor"]
        if "lidar_aug_matrix" not in data:
            data["lidar_aug_matrix"] = np.eye(4)
        data["lidar_aug_matrix"] = lidar_augs @ data["lidar_aug_matrix"]
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class BEVFusionRandomFlip3D:
    """Two coin flips: horizontal negates y, vertical negates x, of the points, the boxes (with their yaw and velocity) and the
    BEV masks; both compose into `lidar_aug_matrix`.  The two draws are also recorded as `pcd_horizontal_flip` /
    `pcd_vertical_flip` (RandomFlip3D's keys; the reference's BEVFusion class keeps them to itself)."""

    def __init__(self, defer=False):
        self.defer = bool(defer)

    def transform(self, data):
        flip_horizontal = np.random.choice([0, 1])
        flip_vertical = np.random.choice([0, 1])
        rotation = np.eye(3)
        b = None
        if "gt_bboxes_3d" in data:
            b, was_array = _unwrap(data["gt_bboxes_3d"])
        if flip_horizontal:
            rotation = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1]]) @ rotation
            if b is not None:
                b[:, 1::7] = -b[:, 1::7]
                b[:, 6] = -b[:, 6]
            if "gt_masks_bev" in data:
                data["gt_masks_bev"] = data["gt_masks_bev"][:, :, ::-1].copy()
        if flip_vertical:
            rotation = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, 1]]) @ rotation
            if b is not None:
                b[:, 0::7] = -b[:, 0::7]
                b[:, 6] = -b[:, 6] + np.pi
            if "gt_masks_bev" in data:
                data["gt_masks_bev"] = data["gt_masks_bev"][:, ::-1, :].copy()
        if b is not None:
            data["gt_bboxes_3d"] = _wrap(b, was_array)
        if "points" in data:
            if self.defer:
                _plan_of(data).set_flip(flip_horizontal, flip_vertical)
            else:
                _apply(data, PointsAugPlan().set_flip(flip_horizontal, flip_vertical))
        if "lidar_aug_matrix" not in data:
            data["lidar_aug_matrix"] = np.eye(4)
        data["lidar_aug_matrix"][:3, :] = rotation @ data["lidar_aug_matrix"][:3, :]
        data["pcd_horizontal_flip"], data["pcd_vertical_flip"] = bool(flip_horizontal), bool(flip_vertical)
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class PointsRangeFilter:
    """Keeps the points strictly inside point_cloud_range (x, y, z minimum, then maximum), in their order."""

    def __init__(self, point_cloud_range, defer=False):
        self.pcd_range = np.array(point_cloud_range, dtype=np.float32)
        self.defer = bool(defer)

    def transform(self, data):
        if self.defer:
            _plan_of(data).set_range(self.pcd_range)
            return data
        mask = _apply(data, PointsAugPlan().set_range(self.pcd_range)).numpy()
        for key in ("pts_instance_mask", "pts_semantic_mask"):
            if data.get(key) is not None:
                data[key] = data[key][mask]
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class ObjectRangeFilter:
    """Keeps the boxes whose centre lies strictly inside the BEV range and wraps their yaw into [-pi, pi)."""

    def __init__(self, point_cloud_range):
        self.pcd_range = np.array(point_cloud_range, dtype=np.float32)

    def transform(self, data):
        b, was_array = _unwrap(data["gt_bboxes_3d"])
        r = self.pcd_range[[0, 1, 3, 4]]
        mask = (b[:, 0] > r[0]) & (b[:, 1] > r[1]) & (b[:, 0] < r[2]) & (b[:, 1] < r[3])
        b = b[mask]
        labels = data["gt_labels_3d"]
        data["gt_labels_3d"] = labels[mask] if torch.is_tensor(labels) else np.asarray(labels)[mask.numpy().astype(bool)]
        period = 2 * np.pi  # limit_yaw(offset=0.5, period=2 pi)
        b[:, 6] = b[:, 6] - torch.floor(b[:, 6] / period + 0.5) * period
        data["gt_bboxes_3d"] = _wrap(b, was_array)
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class ObjectNameFilter:
    """Keeps the boxes whose label is one of range(len(classes))."""

    def __init__(self, classes):
        self.classes = classes
        self.labels = list(range(len(self.classes)))

    def transform(self, data):
        labels = data["gt_labels_3d"]
        keep = np.array([int(n) in self.labels for n in labels], dtype=bool)
        boxes = data["gt_bboxes_3d"]
        if torch.is_tensor(boxes):
            data["gt_bboxes_3d"] = boxes[torch.from_numpy(keep)]
        else:
            data["gt_bboxes_3d"] = np.asarray(boxes)[keep]
        data["gt_labels_3d"] = labels[torch.from_numpy(keep)] if torch.is_tensor(labels) else np.asarray(labels)[keep]
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class PointShuffle:
    """defer=False: points[torch.randperm(n)], as the reference.  defer=True: one torch.randint for the plan's 64-bit seed; the
    order is shuffle_permutation(seed, number of points the filter kept)."""

    def __init__(self, defer=False):
        self.defer = bool(defer)

    def transform(self, data):
        if self.defer:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            _plan_of(data).set_shuffle(seed)
            return data
        pts = data["points"]
        idx = torch.randperm(len(pts))
        data["points"] = pts[idx.numpy()] if isinstance(pts, np.ndarray) else pts[idx]
        for key in ("pts_instance_mask", "pts_semantic_mask"):
            if data.get(key) is not None:
                data[key] = data[key][idx.numpy()]
        return data

    __call__ = transform


from . import object_sample  # noqa: E402,F401  registers ObjectSample and DataBaseSampler beside the chain
from . import loading  # noqa: E402,F401  registers LoadPointsFromFile and LoadPointsFromMultiSweeps in front of it
