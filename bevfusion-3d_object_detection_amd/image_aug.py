"""ImageAug3D (BF/transforms_3d.py:13-127): resize, crop, mirror and rotate each camera frame and record the 4 x 4
`img_aug_matrix` the view transform consumes.  The reference does the pixels with PIL on the host: `resize` (bicubic, a = -0.5,
antialiased, one pass per axis with a uint8 image in between), `crop` (zero outside), `transpose(FLIP_LEFT_RIGHT)` and `rotate`
(nearest neighbour about the centre, zero outside).  All of it is integer arithmetic on uint8 pixels, restated here so that the
result is PIL's bit for bit:

  resize, per axis:  out[i] = clamp((2^21 + sum_j px[lo_i + j] * k_ij) >> 22, 0, 255), k_ij the bicubic weights of output i
                     normalised in double and rounded to 22 fractional bits (`coefficients`)
  rotate:            out[Y, X] = in[(a5 + X a3 + Y a4) >> 16, (a2 + X a0 + Y a1) >> 16], 16.16 fixed point (`rotation_terms`)

Three ways to the pixels:
  * `torch_image_aug(frames, plan)`: plain torch, any device, integers only -- the baseline, the fallback and the yardstick;
  * `ImageAug3D(..., defer=False).transform(data)`: what the reference does, through the torch path on the host;
  * `ImageAug3D(..., defer=True)`: the host only samples the parameters, builds the resampling tables of the draw (where the plan
    is made, i.e. in the loader's worker: `sample_tables`) and writes `img_aug_matrix` and `img_aug_plan`; the raw
    uint8 frames travel to the device and Det3DDataPreprocessor runs `fused_image_aug` (csrc/image_aug.hip): resize + crop +
    flip into a uint8 intermediate, then rotate + normalise + pad + cast -- two launches and one table upload per batch.

GridMask (BF/transforms_3d.py:204-288), the step behind it in the camera + LiDAR train_pipeline (ImageAug3D -> the LiDAR chain of
points_aug.py -> GridMask -> PointShuffle), is here as well: one mask of bands per sample, a closed form of the drawn integers
(`grid_mask_params`, `torch_grid_mask`: PIL's rotated canvas bit for bit through the same `rotation_terms`).  defer=False
multiplies the augmented float32 frames as the reference does; defer=True puts the record on the plan (`AugPlan.grid_mask`) and
both deferred paths apply it to the uint8 result before normalise and pad -- `torch_image_aug`, and on the device the finish
kernel of `fused_image_aug` (bfhip_image_aug_masked), without a further launch, upload or buffer.

BFHIP_IMG_AUG (ships on; measured with tools/image_aug_micro.py: DESIGN.md section 6): 0 sends every deferred
batch through `torch_image_aug` + the preprocessor's own path.  CPU tensors, non-contiguous frames and plans above the
kernel's tap bound go that way as well.  PATHS counts the deferred batches each way took.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from .registry import TRANSFORMS

ENABLED = os.environ.get("BFHIP_IMG_AUG", "1") != "0"
PATHS = {"kernel": 0, "torch": 0}  # deferred image batches taken by each path (tests, tools)

PRECISION_BITS = 22  # PIL's fixed point for the resampling weights
PLAN_COLUMNS = ("newW", "newH", "crop_x", "crop_y", "flip", "rotates", "a0", "a1", "a2", "a3", "a4", "a5")


# GridMask's record of one sample (bfhip_grid_mask, include/bevfusion_hip.h): the canvas is hh x ww, bands of `length` every `d`
# from st_h / st_w on, the fH x fW window starts at (oy, ox), and the canvas is rotated by r degrees through a0 .. a5
GRID_MASK_COLUMNS = ("active", "d", "length", "st_h", "st_w", "use_h", "use_w", "mode", "hh", "ww", "oy", "ox", "r", "rotates",
                     "a0", "a1", "a2", "a3", "a4", "a5")


class AugPlan(np.ndarray):
    """int32[N, 12] (PLAN_COLUMNS), one row per camera, with the output size as the attribute `final_dim` = (fH, fW).  A numpy
    array, so that Det3DDataPreprocessor.cast_data leaves it on the host.  `tables` (None, or what `sample_tables` made: the
    resampling tables of the sample's cameras for one source size) travels with the object through pickling, not through
    slicing or copies; rows are not to be edited once it is set.  `grid_mask` (None, or the sample's int32[20] record of
    GridMask(defer=True): GRID_MASK_COLUMNS) travels through pickling, slicing and copies: the mask is the sample's."""

    def __new__(cls, rows, final_dim):
        obj = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, len(PLAN_COLUMNS)).view(cls)
        obj.final_dim = (int(final_dim[0]), int(final_dim[1]))
        return obj

    def __array_finalize__(self, obj):
        self.final_dim = getattr(obj, "final_dim", None)
        self.tables = None
        self.grid_mask = getattr(obj, "grid_mask", None)

    def __reduce__(self):  # keep final_dim, the tables and the mask record through pickling (loader workers)
        fn, args, state = super().__reduce__()
        return fn, args, (state, self.final_dim, self.tables, self.grid_mask)

    def __setstate__(self, state):
        super().__setstate__(state[0])
        self.final_dim, self.tables = state[1], state[2]
        self.grid_mask = state[3] if len(state) > 3 else None  # a pickle from before the record existed


# ---------------------------------------------------------------------------------------------- PIL's arithmetic on the host
def _bicubic(x):
    x = np.abs(x)
    a = -0.5
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


_coeff_cache = collections.OrderedDict()  # least recently used first
_COEFF_CACHE_ENTRIES = 64         # a test pipeline needs two; a training draw is a new key nearly every time


def coefficients(in_size, out_size, first=0, count=None):
    """PIL's resampling table of one axis for the outputs [first, first + count): (lo int32[count], n int32[count],
    k int32[count, taps]) with out[i] = clamp((2^21 + sum_{j < n_i} px[lo_i + j] * k_ij) >> 22); k is zero beyond n_i and taps is
    the largest n_i.  Built in double as PIL builds it; the last 64 distinct (in_size, out_size, first, count) are kept."""
    count = out_size - first if count is None else count
    key = (int(in_size), int(out_size), int(first), int(count))
    hit = _coeff_cache.get(key)
    if hit is not None:
        _coeff_cache.move_to_end(key)
        return hit
    in_size, out_size, first, count = key
    if not (in_size >= 1 and out_size >= 1 and first >= 0 and count >= 0 and first + count <= out_size):
        raise ValueError("coefficients: in=%d out=%d first=%d count=%d" % key)
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = hi - lo
    ss = 1.0 / fs
    j = np.arange(ksize, dtype=np.int64)[None, :]
    w = _bicubic((j + lo[:, None] - center[:, None] + 0.5) * ss)
    w = np.where(j < n[:, None], w, 0.0)
    ww = np.zeros(count, np.float64)
    for t in range(ksize):  # PIL sums left to right
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.trunc(np.where(w < 0, -0.5, 0.5) + w * (1 << PRECISION_BITS)).astype(np.int32)
    taps = int(n.max()) if count else 0
    out = (lo.astype(np.int32), n.astype(np.int32), np.ascontiguousarray(k[:, :taps]))
    _coeff_cache[key] = out
    while len(_coeff_cache) > _COEFF_CACHE_ENTRIES:
        _coeff_cache.popitem(last=False)
    return out


def rotation_terms(angle, w, h):
    """(rotates, [a0 .. a5]): PIL's `rotate(angle)` of a w x h image as the 16.16 fixed-point affine of its nearest-neighbour
    transform, from the double-precision angle.  rotates = 0: the image is copied."""
    angle = float(angle) % 360.0
    if angle == 0.0:
        return 0, [65536, 0, 0, 0, 65536, 0]
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + cx
    m[5] = m[3] * -cx + m[4] * -cy + cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    a = [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    return 1, [_wrap32(v) for v in a]


def _wrap32(v):
    return (int(v) + (1 << 31)) % (1 << 32) - (1 << 31)


def make_plan(params, final_dim):
    """params: per camera (resize, resize_dims, crop, flip, rotate) as sample_augmentation returns them -> AugPlan."""
    fH, fW = int(final_dim[0]), int(final_dim[1])
    rows = []
    for _, dims, crop, flip, rotate in params:
        if int(crop[2]) - int(crop[0]) != fW or int(crop[3]) - int(crop[1]) != fH:
            raise ValueError("crop %r is not final_dim %r" % (tuple(crop), (fH, fW)))
        rotates, a = rotation_terms(rotate, fW, fH)
        rows.append([int(dims[0]), int(dims[1]), int(crop[0]), int(crop[1]), int(bool(flip)), rotates] + a)
    return AugPlan(np.array(rows, dtype=np.int64).astype(np.int32), (fH, fW))


def aug_matrix(resize, crop, flip, rotate):
    """The 4 x 4 float32 img_aug_matrix of one camera: the reference's float32 torch operations in the reference's order
    (BF/transforms_3d.py:73-91, :113-115)."""
    rotation = torch.eye(2)
    translation = torch.zeros(2)
    rotation *= resize
    translation -= torch.Tensor(crop[:2])
    if flip:
        A = torch.Tensor([[-1, 0], [0, 1]])
        b = torch.Tensor([crop[2] - crop[0], 0])
        rotation = A.matmul(rotation)
        translation = A.matmul(translation) + b
    theta = rotate / 180 * np.pi
    A = torch.Tensor([[np.cos(theta), np.sin(theta)], [-np.sin(theta), np.cos(theta)]])
    b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    b = A.matmul(-b) + b
    rotation = A.matmul(rotation)
    translation = A.matmul(translation) + b
    out = torch.eye(4)
    out[:2, :2] = rotation
    out[:2, 3] = translation
    return out.numpy()


# ---------------------------------------------------------------------------------------------- the plain-torch path
def _window(first, size, limit):
    """[first, first + size) cut to [0, limit): (start in the resized image, count, offset in the crop)."""
    lo, hi = max(first, 0), min(first + size, limit)
    return (lo, hi - lo, lo - first) if hi > lo else (0, 0, 0)


def _resample_axis(x, axis, table, dev):
    """x uint8 [rows, cols, 3] resampled along `axis` by a `coefficients` table, whose lo is relative to x's own origin."""
    lo, n, k = table
    taps = k.shape[1]
    lo_t = torch.from_numpy(lo.astype(np.int64)).to(dev)
    k_t = torch.from_numpy(k).to(dev)
    idx = (lo_t[:, None] + torch.arange(taps, device=dev)[None, :]).clamp_(max=x.shape[axis] - 1)  # k is 0 where clamped
    g = x.index_select(axis, idx.reshape(-1)).to(torch.int32)
    if axis == 1:
        g = g.view(x.shape[0], len(lo), taps, 3) * k_t[None, :, :, None]
        acc = g.sum(2, dtype=torch.int32)
    else:
        g = g.view(len(lo), taps, x.shape[1], 3) * k_t[:, :, None, None]
        acc = g.sum(1, dtype=torch.int32)
    return ((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS).clamp_(0, 255).to(torch.uint8)


def _augment_one(frame, row, fH, fW):
    """frame uint8 [H, W, 3] -> uint8 [fH, fW, 3]."""
    dev = frame.device
    H, W = int(frame.shape[0]), int(frame.shape[1])
    newW, newH, crop_x, crop_y, flip, rotates = (int(v) for v in row[:6])
    out = torch.zeros((fH, fW, 3), dtype=torch.uint8, device=dev)
    x0, nx, ox = _window(crop_x, fW, newW)
    y0, ny, oy = _window(crop_y, fH, newH)
    if nx > 0 and ny > 0:
        hlo, hn, hk = coefficients(W, newW, x0, nx)
        vlo, vn, vk = coefficients(H, newH, y0, ny)
        r0, r1 = int(vlo.min()), int((vlo + vn).max())  # the source rows and columns the crop needs
        c0, c1 = int(hlo.min()), int((hlo + hn).max())
        src = frame[r0:r1, c0:c1]
        mid = _resample_axis(src, 1, (hlo - c0, hn, hk), dev)
        out[oy:oy + ny, ox:ox + nx] = _resample_axis(mid, 0, (vlo - r0, vn, vk), dev)
    if flip:
        out = out.flip(1)
    if rotates:
        a = [int(v) for v in row[6:12]]
        X = torch.arange(fW, dtype=torch.int32, device=dev)[None, :]
        Y = torch.arange(fH, dtype=torch.int32, device=dev)[:, None]
        sx = (X * a[0] + Y * a[1] + a[2]) >> 16  # int32: wraps as C does
        sy = (X * a[3] + Y * a[4] + a[5]) >> 16
        inside = (sx >= 0) & (sx < fW) & (sy >= 0) & (sy < fH)
        flat = (sy.clamp(0, fH - 1).long() * fW + sx.clamp(0, fW - 1).long()).reshape(-1)
        out = out.reshape(fH * fW, 3).index_select(0, flat).view(fH, fW, 3) * inside[:, :, None].to(torch.uint8)
    return out


def _as_u8_frames(frames):
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    elif isinstance(frames, (list, tuple)):
        frames = torch.stack([torch.as_tensor(np.ascontiguousarray(f) if isinstance(f, np.ndarray) else f) for f in frames])
    if frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError("frames must be [N, H, W, 3], got %s" % (tuple(frames.shape),))
    if frames.dtype == torch.float32:
        frames = frames.to(torch.uint8)  # integer-valued floats, as the reference's astype("uint8")
    if frames.dtype != torch.uint8:
        raise TypeError("frames must be uint8 (or float32 holding integers), got %s" % frames.dtype)
    return frames


def _final_dim(plan, final_dim):
    final_dim = final_dim if final_dim is not None else getattr(plan, "final_dim", None)
    if final_dim is None:
        raise ValueError("the plan carries no final_dim (not an AugPlan): pass final_dim=(fH, fW)")
    return int(final_dim[0]), int(final_dim[1])


def torch_image_aug(frames, plan, final_dim=None):
    """frames uint8 [N, H, W, 3] (or float32 holding integers) + AugPlan -> uint8 [N, 3, fH, fW] on frames' device: PIL's
    resize, crop, mirror and rotate in integer torch operations, bit for bit."""
    fH, fW = _final_dim(plan, final_dim)
    frames = _as_u8_frames(frames)
    rows = np.asarray(plan)
    if rows.shape != (frames.shape[0], len(PLAN_COLUMNS)):
        raise ValueError("plan %s does not fit %d frames" % (rows.shape, frames.shape[0]))
    views = [_augment_one(f, r, fH, fW) for f, r in zip(frames, rows)]
    out = torch.stack(views).permute(0, 3, 1, 2).contiguous()
    record = getattr(plan, "grid_mask", None)
    if record is not None and int(record[0]):  # GridMask(defer=True): one mask for every camera of the sample
        out *= torch_grid_mask(record, fH, fW, out.device)
    return out


# ---------------------------------------------------------------------------------------------- GridMask's mask
def grid_mask_params(h, w, d, length, st_h, st_w, r, use_h=True, use_w=True, mode=0):
    """The int32[20] record (GRID_MASK_COLUMNS) of one drawn mask on h x w images: the reference's canvas of int(1.5 h) x
    int(1.5 w), its centre window and PIL's `rotate(r)` of that canvas as `rotation_terms`.  d .. r are the drawn integers."""
    hh, ww = int(1.5 * h), int(1.5 * w)
    rotates, a = rotation_terms(int(r), ww, hh)
    rec = [1, int(d), int(length), int(st_h), int(st_w), int(bool(use_h)), int(bool(use_w)), int(mode == 1), hh, ww,
           (hh - int(h)) // 2, (ww - int(w)) // 2, int(r), rotates] + a
    return np.array(rec, dtype=np.int64).astype(np.int32)


def torch_grid_mask(record, h, w, device=None):
    """uint8 [h, w] of 0 / 1: what the reference multiplies the frames by, in integer torch operations.  Canvas point (Y, X) is
    0 when it lies in a band -- t = Y - st_h >= 0, t // d < hh // d and t % d < length with use_h; X, st_w and ww likewise with
    use_w -- and 1 otherwise; output (y, x) reads the canvas at (y + oy, x + ox) moved through the rotation's 16.16 affine as
    `_augment_one` does, 0 outside the canvas; mode 1 inverts.  An inactive record gives ones."""
    rec = dict(zip(GRID_MASK_COLUMNS, (int(v) for v in record)))
    if not rec["active"]:
        return torch.ones((h, w), dtype=torch.uint8, device=device)
    Y = torch.arange(h, dtype=torch.int32, device=device)[:, None] + rec["oy"]
    X = torch.arange(w, dtype=torch.int32, device=device)[None, :] + rec["ox"]
    inside = None
    if rec["rotates"]:
        sx = (X * rec["a0"] + Y * rec["a1"] + rec["a2"]) >> 16  # int32: wraps as C does
        sy = (X * rec["a3"] + Y * rec["a4"] + rec["a5"]) >> 16
        inside = (sx >= 0) & (sx < rec["ww"]) & (sy >= 0) & (sy < rec["hh"])
        X, Y = sx.clamp(0, rec["ww"] - 1), sy.clamp(0, rec["hh"] - 1)
    d, length = rec["d"], rec["length"]

    def band(v, start, size):
        t = v - start
        tc = t.clamp(min=0)
        return (t >= 0) & (torch.div(tc, d, rounding_mode="floor") < size // d) & (tc % d < length)

    masked = torch.zeros((h, w), dtype=torch.bool, device=device)
    if rec["use_h"]:
        masked = masked | band(Y, rec["st_h"], rec["hh"])
    if rec["use_w"]:
        masked = masked | band(X, rec["st_w"], rec["ww"])
    keep = ~masked if inside is None else inside & ~masked
    if rec["mode"]:
        keep = ~keep
    return keep.to(torch.uint8)


# ---------------------------------------------------------------------------------------------- the fused device path
class _Cam(ctypes.Structure):
    """bfhip_image_aug_cam (include/bevfusion_hip.h)."""
    _fields_ = [("data", ctypes.c_void_p), ("h", ctypes.c_int), ("w", ctypes.c_int), ("crop", ctypes.c_int * 2),
                ("flip", ctypes.c_int), ("rotates", ctypes.c_int), ("a", ctypes.c_int * 6),
                ("h_off", ctypes.c_int), ("h_taps", ctypes.c_int), ("h_first", ctypes.c_int), ("h_count", ctypes.c_int),
                ("v_off", ctypes.c_int), ("v_taps", ctypes.c_int), ("v_first", ctypes.c_int), ("v_count", ctypes.c_int)]


def sample_tables(plan, H, W, final_dim=None):
    """The resampling tables of one sample's cameras on H x W frames: ((H, W), int32 buffer, per camera (h_off, h_taps, h_first,
    h_count, v_off, v_taps, v_first, v_count)).  Per camera the horizontal and vertical table of its crop window, each distinct
    one stored once; entry i of a table is (lo, n, k_0 .. k_{taps-1}).  Kept on the AugPlan (`plan.tables`): ImageAug3D(defer=True)
    calls this where the plan is made -- in the loader's worker, a new (resize, crop) is a new table -- and the consumer finds
    it there; a plan that arrives without (or for another source size) gets it on first use."""
    made = getattr(plan, "tables", None)
    if made is not None and made[0] == (H, W):
        return made
    fH, fW = _final_dim(plan, final_dim)
    parts, where, refs, used = [], {}, [], 0
    for row in np.asarray(plan):
        ref = []
        for in_size, out_size, first, size in ((W, int(row[0]), int(row[2]), fW), (H, int(row[1]), int(row[3]), fH)):
            start, count, _ = _window(first, size, out_size)
            key = (in_size, out_size, start, count)
            if key not in where:
                lo, n, k = coefficients(*key)
                block = np.concatenate([lo[:, None], n[:, None], k], 1).astype(np.int32).reshape(-1)
                where[key] = (used, k.shape[1])
                parts.append(block)
                used += block.size
            ref += [where[key][0], where[key][1], start, count]
        refs.append(ref)
    buf = np.concatenate(parts) if used else np.zeros(0, np.int32)
    made = ((H, W), np.ascontiguousarray(buf, dtype=np.int32), refs)
    if isinstance(plan, AugPlan):
        plan.tables = made
    return made


def _pack_tables(shapes, plans, fH, fW):
    """The batch's one table buffer: the samples' buffers end to end, the cameras' offsets moved along:
    (int32 buffer, per-camera (h_off, h_taps, h_first, h_count, v_off, v_taps, v_first, v_count))."""
    parts, refs, used = [], [], 0
    for (H, W), plan in zip(shapes, plans):
        _, buf, sample_refs = sample_tables(plan, H, W, (fH, fW))
        refs += [[r[0] + used, r[1], r[2], r[3], r[4] + used, r[5], r[6], r[7]] for r in sample_refs]
        parts.append(buf)
        used += buf.size
    return (np.concatenate(parts) if used else np.zeros(1, np.int32)), refs


def fused_supported(frames, plans, final_dim=None):
    """True when bfhip_image_aug takes this batch: device uint8 [N, H, W, 3] contiguous blocks, one view count, and every
    table within the kernel's tap bound."""
    if not frames or not all(torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 and f.dim() == 4 and f.shape[-1] == 3
                             and f.is_contiguous() and f.device == frames[0].device and f.shape[0] == frames[0].shape[0]
                             for f in frames):
        return False
    fH, fW = _final_dim(plans[0], final_dim)
    lib = _lib.load()
    for f, plan in zip(frames, plans):
        H, W = int(f.shape[1]), int(f.shape[2])
        refs = sample_tables(plan, H, W, (fH, fW))[2]
        for row, r in zip(np.asarray(plan), refs):
            if not lib.bfhip_image_aug_supported(H, W, int(row[1]), int(row[0]), fH, fW, r[1] if r[3] else 0, r[5] if r[7] else 0):
                return False
    return True


def descriptors(frames, plans, fH, fW):
    """(bfhip_image_aug_cam array, int32 table buffer) of a batch: what bfhip_image_aug takes besides the buffers."""
    B, N = len(frames), int(frames[0].shape[0])
    tables, refs = _pack_tables([(int(f.shape[1]), int(f.shape[2])) for f in frames], plans, fH, fW)
    cams = (_Cam * (B * N))()
    i = 0
    for f, plan in zip(frames, plans):
        H, W = int(f.shape[1]), int(f.shape[2])
        base = f.data_ptr()
        for v, row in enumerate(np.asarray(plan)):
            c = cams[i]
            c.data, c.h, c.w = base + v * H * W * 3, H, W
            c.crop[0], c.crop[1], c.flip, c.rotates = int(row[2]), int(row[3]), int(row[4]), int(row[5])
            for t in range(6):
                c.a[t] = int(row[6 + t])
            (c.h_off, c.h_taps, c.h_first, c.h_count, c.v_off, c.v_taps, c.v_first, c.v_count) = refs[i]
            i += 1
    return cams, tables


def fused_image_aug(frames, plans, final_dim=None, mean_std=None, swap=False, pad_size_divisor=1, pad_value=0,
                    out_dtype=None, channels_last=False, store=None, mid=None):
    """frames: list (one per sample) of device uint8 [N, H, W, 3]; plans: list of AugPlan -> the batch [B, N, 3, H', W'] in every
    form Det3DDataPreprocessor writes.  Two launches (resize + crop + flip into a uint8 intermediate; rotate + normalise + pad +
    cast) and one table upload; no synchronisation.  Plans with an active GridMask record (`plan.grid_mask`) have their sample's
    pixels masked in the second launch, the records travelling in its arguments.  store / mid: preallocated flat device buffers for the batch (B * N * 3 *
    H' * W' elements of the output dtype) and the uint8 intermediate (B * N * 3 * fH * fW) instead of fresh ones (tools, tests)."""
    fH, fW = _final_dim(plans[0], final_dim)
    B, N, dev = len(frames), int(frames[0].shape[0]), frames[0].device
    Hp = (fH + pad_size_divisor - 1) // pad_size_divisor * pad_size_divisor
    Wp = (fW + pad_size_divisor - 1) // pad_size_divisor * pad_size_divisor
    cams, tables = descriptors(frames, plans, fH, fW)
    dtype = torch.bfloat16 if out_dtype == torch.bfloat16 else torch.float32
    if store is None:
        store = torch.empty(B * N * 3 * Hp * Wp, dtype=dtype, device=dev)
    if mid is None:
        mid = torch.empty(B * N * 3 * fH * fW, dtype=torch.uint8, device=dev)
    if (store.dtype != dtype or store.numel() != B * N * 3 * Hp * Wp or mid.dtype != torch.uint8
            or mid.numel() != B * N * 3 * fH * fW or not (store.is_contiguous() and mid.is_contiguous())):
        raise ValueError("fused_image_aug: store / mid do not fit the batch")
    if channels_last:
        out = store.view(B * N, Hp, Wp, 3).permute(0, 3, 1, 2).view(B, N, 3, Hp, Wp)
    else:
        out = store.view(B, N, 3, Hp, Wp)
    tables_dev = torch.from_numpy(tables).pin_memory().to(dev, non_blocking=True)  # the batch's one upload
    normalise = mean_std is not None
    mean, std = (_lib.host_f32(v) for v in mean_std) if normalise else (None, None)
    masks = mask_records(plans)
    with torch.cuda.device(dev):
        _lib.call("bfhip_image_aug_masked", cams, None if masks is None else masks.ctypes.data, B, N, tables.ctypes.data,
                  tables_dev.data_ptr(), int(tables.size), fH, fW, mid.data_ptr(), int(bool(swap)), int(normalise), mean, std,
                  float(pad_value), Hp, Wp, 1 if dtype == torch.bfloat16 else 0, int(bool(channels_last)), store.data_ptr(),
                  _lib.stream_of(store))
    return out


def mask_records(plans):
    """The batch's GridMask records as bfhip_image_aug_masked takes them: int32 [B, 20], zeros (inactive) for a sample without
    one; None when no sample has an active one."""
    masks = np.zeros((len(plans), len(GRID_MASK_COLUMNS)), dtype=np.int32)
    for i, plan in enumerate(plans):
        record = getattr(plan, "grid_mask", None)
        if record is not None:
            masks[i] = record
    return masks if masks[:, 0].any() else None


# ---------------------------------------------------------------------------------------------- the transform
@TRANSFORMS.register_module()
class ImageAug3D:
    """The reference's ImageAug3D.  defer=False: `data["img"]` (a list of [H, W, 3] arrays) becomes the list of augmented
    float32 [fH, fW, 3] arrays and `data["img_aug_matrix"]` the list of [4, 4] matrices.  defer=True: the pixels are left alone
    and `data["img_aug_plan"]` (AugPlan) is written next to `img_aug_matrix` for Det3DDataPreprocessor to run on the device."""

    def __init__(self, final_dim, resize_lim, bot_pct_lim, rot_lim, rand_flip, is_train, defer=False):
        self.final_dim = final_dim
        self.resize_lim = resize_lim
        self.bot_pct_lim = bot_pct_lim
        self.rand_flip = rand_flip
        self.rot_lim = rot_lim
        self.is_train = is_train
        self.defer = bool(defer)

    def sample_augmentation(self, results, camera_index):
        """(resize, resize_dims, crop, flip, rotate) with the reference's np.random calls in the reference's order."""
        H, W = results["ori_shape"]
        fH, fW = self.final_dim
        cam2img = results["cam2img"][camera_index]
        fx, fy, cx, cy = cam2img[0, 0], cam2img[1, 1], cam2img[0, 2], cam2img[1, 2]
        r31, r32, r33 = results["cam2lidar"][camera_index, 2, :3]
        # the image row of the horizon at the left and right edge: nothing above it is cropped in
        yl = cy + cx * (fy / fx) * (r31 / r32) - fy * (r33 / r32)
        yr = cy + (cx - W + 1) * (fy / fx) * (r31 / r32) - fy * (r33 / r32)
        yh = max(0, min(yr, yl))
        if self.is_train:
            resize = np.random.uniform(*self.resize_lim)
        else:
            resize = np.mean(self.resize_lim)
        newW, newH = int(W * resize), int(H * resize)
        crop_h = int(min(newH - fH, yh * resize))
        if self.is_train:
            crop_w = int(np.random.uniform(0, max(0, newW - fW)))
            flip = bool(self.rand_flip and np.random.choice([0, 1]))
            rotate = np.random.uniform(*self.rot_lim)
        else:
            crop_w = int(max(0, newW - fW) / 2)
            flip = False
            rotate = 0
        return resize, (newW, newH), (crop_w, crop_h, crop_w + fW, crop_h + fH), flip, rotate

    def transform(self, data):
        imgs = data["img"]
        params = [self.sample_augmentation(data, i) for i in range(len(imgs))]
        data["img_aug_matrix"] = [aug_matrix(p[0], p[2], p[3], p[4]) for p in params]
        plan = make_plan(params, self.final_dim)
        if self.defer:
            H, W = data["ori_shape"]
            sample_tables(plan, int(H), int(W))  # built here, with the plan: the consumer only joins the samples' buffers
            data["img_aug_plan"] = plan
            return data
        out = []
        for i, img in enumerate(imgs):  # frames of one sample may differ in size
            frame = torch.as_tensor(np.ascontiguousarray(img))[None]
            aug = torch_image_aug(frame, plan[i:i + 1])[0]
            out.append(aug.permute(1, 2, 0).numpy().astype(np.float32))
        data["img"] = out
        return data

    __call__ = transform


@TRANSFORMS.register_module()
class GridMask:
    """The reference's GridMask (BF/transforms_3d.py:204-288) under its keywords: with probability `prob` every camera of the
    sample is multiplied by one drawn mask of bands.  The np.random calls are the reference's, in its order and number, the one
    draw of a skipped sample included.  defer=False: `data["img"]` (float32 [h, w, 3] arrays, after ImageAug3D) is multiplied
    on the host.  defer=True (behind ImageAug3D(defer=True)): the drawn record goes onto `data["img_aug_plan"]`
    (`plan.grid_mask`) and the deferred image path applies it, in the kernel that normalises and pads.

    offset=True is not restated: the reference multiplies a [h, w, 1] numpy mask by a [h, w] torch tensor there, which only
    broadcasts for square images."""

    def __init__(self, use_h, use_w, max_epoch, rotate=1, offset=False, ratio=0.5, mode=0, prob=1.0, fixed_prob=False,
                 defer=False):
        if offset:
            raise NotImplementedError("GridMask: offset=True is not supported: the reference's own code for it fails on every "
                                      "image that is not square (a [h, w, 1] mask times a [h, w] plane)")
        self.use_h = use_h
        self.use_w = use_w
        self.rotate = rotate
        self.offset = offset
        self.ratio = ratio
        self.mode = mode
        self.st_prob = prob
        self.prob = prob
        self.epoch = None
        self.max_epoch = max_epoch
        self.fixed_prob = fixed_prob
        self.defer = bool(defer)

    def set_epoch(self, epoch):
        self.epoch = epoch
        if not self.fixed_prob:
            self.set_prob(self.epoch, self.max_epoch)

    def set_prob(self, epoch, max_epoch):
        self.prob = self.st_prob * epoch / max_epoch

    def sample(self, h, w):
        """The record of one applied draw on h x w images: the reference's calls after its first."""
        d = np.random.randint(2, min(h, w))
        if self.ratio == 1:
            length = np.random.randint(1, d)
        else:
            length = min(max(int(d * self.ratio + 0.5), 1), d - 1)
        st_h = np.random.randint(d)
        st_w = np.random.randint(d)
        r = np.random.randint(self.rotate)
        return grid_mask_params(h, w, d, length, st_h, st_w, r, self.use_h, self.use_w, self.mode)

    def transform(self, results):
        plan = results.get("img_aug_plan")
        if self.defer and plan is None:
            raise ValueError("GridMask(defer=True) needs the img_aug_plan of ImageAug3D(defer=True) in front of it; on "
                             "augmented frames use defer=False")
        if not self.defer and plan is not None:
            raise ValueError("GridMask(defer=False) behind ImageAug3D(defer=True): the frames are still raw and the mask "
                             "would be drawn at the wrong size; use defer=True")
        if np.random.rand() > self.prob:
            return results
        if self.defer:
            plan.grid_mask = self.sample(*plan.final_dim)
            return results
        imgs = results["img"]
        h, w = imgs[0].shape[0], imgs[0].shape[1]
        mask = torch_grid_mask(self.sample(h, w), h, w).numpy().astype(np.float32)[:, :, None]
        results.update(img=[x * mask for x in imgs])
        return results

    __call__ = transform
