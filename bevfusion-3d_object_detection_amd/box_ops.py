"""Points in rotated boxes, per box: the reference's box_np_ops.points_in_rbbox (M3D/structures/ops/box_np_ops.py:354-377) and
the per-box gathers its ground-truth database builder makes of it (tools/dataset_converters/create_gt_database.py:257, 296-297).

    counts, rows = points_in_boxes(points, boxes, center=True)

`points` is float32 [n, C] (3 <= C <= 8), `boxes` float32 [K, 7+] in LiDAR convention (x, y, z of the bottom centre, dx, dy, dz,
yaw; further columns are ignored).  `counts` is int32 [K], `rows` float32 [sum(counts), C], box-major: the rows of box j, in
ascending point index, at [start_j, start_j + counts_j), start the exclusive prefix sum of counts.  A row that lies in two boxes
appears once in each.  With center=True columns 0..2 of a row of box j are point - boxes[j, :3], one float32 subtraction each
(the reference's `gt_points[:, :3] -= gt_boxes_3d[i, :3]`); the other columns are copied.

The bits are DEFINED by `torch_points_in_boxes`, plain torch on any device.  The planes are points_aug.paste_planes(boxes), the
reference's corner -> surface -> plane sequence in the boxes' own float32.  Membership follows the reference's loop
(box_np_ops.py:664-676): row i is in box j UNLESS some plane k has ((x n0 + y n1) + z n2) + d >= 0, every product and sum one
float32 operation.  The test is "not (sign >= 0)", not "sign < 0": a row with a NaN coordinate has NaN signs, is never left,
and is therefore inside EVERY box, as in the reference.  A box with a zero dimension has zero normals on four faces, sign = d = 0
there, and holds nothing (but such NaN rows).  (ObjectSample's paste, points_aug.points_in_any_box, tests sign < 0 and drops no NaN row; the two
differ on NaN rows only.)

On the GPU the operator is csrc/points_in_boxes.hip: bfhip_points_in_boxes_count (count and scan launches), ONE host read of the
K counts -- the output's size is not known before -- and bfhip_points_in_boxes_gather (the ranked write).  No atomics: the same
bytes on every run.  At most max_boxes() boxes per call; above that, for CPU tensors, other dtypes and non-contiguous points, and
with BFHIP_POINTS_IN_BOXES=0, the torch specification runs, same bits.  PATHS counts the calls each way took.

BFHIP_POINTS_IN_BOXES ships on (measured with tools/gt_database_micro.py: DESIGN.md section 6).
"""
import os

import numpy as np
import torch

from . import _lib
from . import points_aug as pa

ENABLED = os.environ.get("BFHIP_POINTS_IN_BOXES", "1") != "0"
PATHS = {"kernel": 0, "torch": 0}  # calls taken by each path (tests, tools)


def max_boxes():
    """The most boxes per call the kernels take (bfhip_points_in_boxes_max_boxes)."""
    return int(_lib.load().bfhip_points_in_boxes_max_boxes())


def _as_boxes(boxes):
    """float32 [K, 7+] array of boxes given as an array, a tensor or anything with `.tensor`."""
    boxes = getattr(boxes, "tensor", boxes)
    if torch.is_tensor(boxes):
        boxes = boxes.detach().cpu().numpy()
    boxes = np.asarray(boxes)
    if boxes.ndim != 2 or boxes.shape[1] < 7:
        raise ValueError("boxes must be [K, 7 or more], got %s" % (boxes.shape,))
    return np.ascontiguousarray(boxes, dtype=np.float32)


def _as_points(points):
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(np.ascontiguousarray(points))
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] < 3:
        raise ValueError("points must be a [n, C] tensor or array with C >= 3")
    return points if points.dtype == torch.float32 else points.to(torch.float32)


def inside_mask(points, planes):
    """bool [K, n]: box-major membership of the rows of `points` (float32 [n, C] tensor) in the boxes of `planes` (float32 [K, 6,
    4] tensor on the same device): not (((x n0 + y n1) + z n2) + d >= 0) for all six planes."""
    n, K = int(points.shape[0]), int(planes.shape[0])
    xyz = points[:, :3].t().contiguous()  # [3, n]: the pairs as [K, n], points along the contiguous axis
    out = torch.empty((K, n), dtype=torch.bool, device=points.device)
    step = 16384 if points.device.type == "cpu" else max(1, min(n, (1 << 26) // max(K, 1)))  # temporaries of bounded size
    for s in range(0, n, step):
        x, y, z = xyz[0:1, s:s + step], xyz[1:2, s:s + step], xyz[2:3, s:s + step]
        left = None
        for k in range(6):
            pl = planes[:, k, :, None]
            ge = (((x * pl[:, 0] + y * pl[:, 1]) + z * pl[:, 2]) + pl[:, 3]) >= 0
            left = ge if left is None else left.logical_or_(ge)
        out[:, s:s + step] = left.logical_not_()
    return out


def torch_points_in_boxes(points, boxes, center=False, return_mask=False):
    """The specification: (counts int32 [K], rows float32 [sum(counts), C]) on the points' device, and with return_mask the bool
    [n, K] membership as well.  See the module docstring; a row with a NaN coordinate is inside every box."""
    p = _as_points(points)
    b = _as_boxes(boxes)
    planes = torch.from_numpy(pa.paste_planes(b)).to(p.device)
    inside = inside_mask(p, planes)
    bi, pi = torch.nonzero(inside, as_tuple=True)  # row-major over [K, n]: box-major, ascending point index
    rows = p[pi]
    if center and rows.shape[0]:
        rows[:, :3] = rows[:, :3] - torch.from_numpy(b[:, :3]).to(p.device)[bi]
    counts = inside.sum(1).to(torch.int32)
    return (counts, rows, inside.t()) if return_mask else (counts, rows)


def kernel_supported(points, n_boxes):
    """True when csrc/points_in_boxes.hip takes this call: a float32 contiguous [n, C] device tensor, 3 <= C <= 8, n < 2^31, at
    most max_boxes() boxes."""
    return (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2
            and points.is_contiguous() and 3 <= points.shape[1] <= 8 and points.shape[0] < (1 << 31) and n_boxes <= max_boxes())


def upload_table(planes, centers, dev):
    """(planes [K, 6, 4], centers [K, 3]) as device views of ONE buffer: packed in one pinned host buffer, one non-blocking copy
    on the current stream."""
    K = int(planes.shape[0])
    host = torch.empty(K * 27, dtype=torch.float32, pin_memory=True)
    if K:
        np.concatenate([planes.reshape(-1), centers.reshape(-1)], out=host.numpy())
    table = torch.empty(K * 27, dtype=torch.float32, device=dev)
    table.copy_(host, non_blocking=True)
    return table[:K * 24].view(K, 6, 4), table[K * 24:].view(K, 3)


def kernel_count(points, planes, want_words=False):
    """Launches 1 and 2 -> (counts int32 [K] on the device, the membership words uint64-as-int64 [n, ceil(K / 64)] or None, the
    workspace the gather needs)."""
    n, C, K, dev = int(points.shape[0]), int(points.shape[1]), int(planes.shape[0]), points.device
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    words = torch.empty((n, (K + 63) // 64), dtype=torch.int64, device=dev) if want_words else None
    nbytes = _lib.call_size("bfhip_points_in_boxes_workspace_bytes", n, K)
    work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)  # the allocator's blocks are 512-byte aligned
    with torch.cuda.device(dev):
        _lib.call("bfhip_points_in_boxes_count", points.data_ptr() if n else None, n, C, planes.data_ptr() if K else None, K,
                  counts.data_ptr() if K else None, words.data_ptr() if want_words and words.numel() else None, work.data_ptr(),
                  nbytes, _lib.stream_of(points))
    return counts, words, (work, nbytes)


def kernel_gather(points, centers, counts, words, work, total, K):
    """Launch 3 -> rows float32 [total, C].  centers: device float32 [K, 3] or None."""
    n, C, dev = int(points.shape[0]), int(points.shape[1]), points.device
    out = torch.empty((total, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.call("bfhip_points_in_boxes_gather", points.data_ptr() if n else None, n, C,
                  centers.data_ptr() if centers is not None and K else None, K, counts.data_ptr() if K else None,
                  words.data_ptr() if words is not None and words.numel() else None, total, out.data_ptr() if total else None, total,
                  work[0].data_ptr(), work[1], _lib.stream_of(points))
    return out


def unpack_words(words, K):
    """bool [n, K] of the kernel's membership words [n, ceil(K / 64)]."""
    j = torch.arange(K, device=words.device)
    return ((words[:, j // 64] >> (j % 64)) & 1).to(torch.bool)


def points_in_boxes(points, boxes, center=False, return_mask=False, counts_to_host=True):
    """(counts, rows[, mask]) as torch_points_in_boxes gives them, through the kernels when they take the call.  `points`: a
    float32 [n, C] tensor (any device) or array; the outputs are tensors on the points' device, except `counts`, which is the
    int32 [K] HOST tensor the call had to read anyway (counts_to_host=False: on the points' device, as the specification)."""
    b = _as_boxes(boxes)
    if not (ENABLED and kernel_supported(points, b.shape[0])):
        PATHS["torch"] += 1
        out = torch_points_in_boxes(points, b, center=center, return_mask=return_mask)
        return ((out[0].cpu(),) + tuple(out[1:])) if counts_to_host else out
    PATHS["kernel"] += 1
    K = int(b.shape[0])
    planes, centers = upload_table(pa.paste_planes(b), b[:, :3], points.device)
    counts, words, work = kernel_count(points, planes, want_words=return_mask)
    host_counts = counts.cpu()  # the call's one host read (it waits for the two launches)
    total = int(host_counts.sum(dtype=torch.int64))
    if total >= (1 << 31):
        raise ValueError("points_in_boxes: %d member rows in all (below 2^31)" % total)
    rows = kernel_gather(points, centers if center else None, counts, words, work, total, K)
    counts = host_counts if counts_to_host else counts
    return (counts, rows, unpack_words(words, K)) if return_mask else (counts, rows)


def points_in_rbbox(points, boxes):
    """box_np_ops.points_in_rbbox(points, rbbox): bool [n, K], True where the point is in the box (z_axis=2, origin=(0.5, 0.5,
    0)).  An array for an array, a tensor on the points' device for a tensor."""
    was_array = isinstance(points, np.ndarray)
    b = _as_boxes(boxes)
    if ENABLED and kernel_supported(points, b.shape[0]):
        PATHS["kernel"] += 1
        planes, _ = upload_table(pa.paste_planes(b), b[:, :3], points.device)
        _, words, _ = kernel_count(points, planes, want_words=True)
        return unpack_words(words, int(b.shape[0]))
    PATHS["torch"] += 1
    p = _as_points(points)
    mask = inside_mask(p, torch.from_numpy(pa.paste_planes(b)).to(p.device)).t()
    return mask.numpy() if was_array else mask
