"""Query initialisation of the TransFusion head (csrc/query_init.hip; BF/bevfusion_head.py:221-260,278-281).

    top_class, top_index, query_pos, query_heatmap_score, rows = query_init(h, flat, K, pos_w, nms_free_classes=())

`h` is the score map `dense_heatmap.detach().sigmoid()`, f32 [B, C, H, W]; `flat` the BEV features [B, Ch, H*W].

The masked map `m` is `h` where the cell is interior (1 <= y <= H-2, 1 <= x <= W-2) and equals the maximum of its 3x3 window in its
own class plane, and 0 elsewhere, borders included; the classes in `nms_free_classes` keep m = h everywhere (upstream mmdet3d's
pedestrian / traffic-cone exception, which the reference has commented out).  The picks are the first K of the C*H*W cells of a
sample ordered by (m descending, flat index c*HW + y*W + x ascending): equal scores go to the lower index, and with fewer than K
positive cells the zero-valued cells follow in ascending flat index.  `torch.topk` leaves both cases open; where it is
unambiguous (distinct scores, at least K positive peaks) the picks are its picks.  A NaN score is never a peak and ranks after
every other cell (in torch it would rank first).

    top_class, top_index   int64 [B, K]      flat index // HW, flat index % HW
    query_pos              f32 [B, K, 2]     (top_index // pos_w + 0.5, top_index % pos_w + 0.5) = the gather from `bev_pos`
    query_heatmap_score    f32 [B, C, K]     m of every class at the picked cell
    rows                   [B, K, Ch]        flat[b, :, top_index[b, p]], dtype of flat; the only differentiable output

Backward of rows: d_flat[b, :, i] = the sum of d_rows[b, p, :] over the picks p of cell i, in ascending p, in f32, rounded once.

`torch_query_init` is the arithmetic in plain torch and the CPU path; `fused_query_init` the three-launch HIP path.  The switch is
BFHIP_QUERY_INIT (read at call time); it ships off (BFHIP_QUERY_INIT=1 turns the kernels on in BEVFusionHead.forward), the
measurements and the open question behind that are in DESIGN.md section 6.
"""
import os

import torch
import torch.nn.functional as F

from . import _lib

DEFAULT = "0"   # ships off: DESIGN.md section 6 "Query initialisation"
LAUNCHES = dict(fwd=0, bwd=0)  # fused calls made so far (tests and tools read the difference)
MAX_K = 512
MAX_CLASSES = 32
_DT = {torch.float32: 0, torch.bfloat16: 1}


def enabled():
    return os.environ.get("BFHIP_QUERY_INIT", DEFAULT) != "0"


def class_mask(nms_free_classes, num_classes):
    """The NMS-free classes as the bit mask the kernel takes."""
    mask = 0
    for c in nms_free_classes:
        if not 0 <= int(c) < num_classes:
            raise ValueError("nms_free_classes: class %r outside [0, %d)" % (c, num_classes))
        mask |= 1 << int(c)
    return mask


def shape_supported(B, C, H, W, K, Ch, nms_kernel_size=3, dtype=torch.float32):
    """Host-only: do the kernels cover these sizes?"""
    return dtype in _DT and bool(_lib.load().bfhip_query_init_supported(B, C, H, W, K, Ch, nms_kernel_size, _DT[dtype]))


def supported(h, flat, K, nms_kernel_size=3, nms_free_classes=()):
    """Does this call run in csrc/query_init.hip?  `flat` must be the channels-last view (its rows [cell, :] contiguous)."""
    if not (h.is_cuda and flat.is_cuda and h.device == flat.device and h.dtype == torch.float32 and flat.dtype in _DT
            and h.dim() == 4 and flat.dim() == 3):
        return False
    B, C, H, W = h.shape
    Ch = flat.shape[1]
    if flat.shape[0] != B or flat.shape[2] != H * W or C > MAX_CLASSES or any(not 0 <= int(c) < C for c in nms_free_classes):
        return False
    if not shape_supported(B, C, H, W, K, Ch, nms_kernel_size, flat.dtype):
        return False
    if any(s < 1 for s, n in zip(h.stride(), h.shape) if n > 1):
        return False
    es = flat.element_size()
    if (Ch > 1 and flat.stride(1) != 1) or flat.stride(2) < Ch or (flat.stride(2) * es) % 16 or flat.data_ptr() % 16:
        return False
    return B == 1 or (flat.stride(0) >= 0 and (flat.stride(0) * es) % 16 == 0)


def masked_scores(h, nms_free_classes=()):
    """m [B, C, H, W] as defined above (3x3 window)."""
    local_max = torch.zeros_like(h)
    local_max[:, :, 1:-1, 1:-1] = F.max_pool2d(h, kernel_size=3, stride=1, padding=0)
    for c in nms_free_classes:
        local_max[:, c] = h[:, c]
    return torch.where((h == local_max) & (h > 0), h, torch.zeros_like(h))


def torch_query_init(h, flat, K, pos_w, nms_free_classes=()):
    """The stated arithmetic in torch ops: runs anywhere, differentiable in `flat` through indexing (a sorted, fixed-order backward)."""
    B, C, H, W = h.shape
    HW = H * W
    class_mask(nms_free_classes, C)
    m = masked_scores(h, nms_free_classes).reshape(B, C, HW)
    rank = torch.where(torch.isnan(h), torch.full_like(h, -1.0), m.view_as(h)).reshape(B, C * HW)
    top = torch.sort(rank, dim=-1, descending=True, stable=True).indices[:, :K]
    top_class, top_index = top // HW, top % HW
    rows = flat.transpose(1, 2)[torch.arange(B, device=flat.device)[:, None], top_index]
    query_pos = torch.stack([(top_index // pos_w).float() + 0.5, (top_index % pos_w).float() + 0.5], dim=-1)
    score = m.gather(index=top_index[:, None, :].expand(-1, C, -1), dim=-1)
    return top_class, top_index, query_pos, score, rows


def _stride(t, d):
    return t.stride(d) if t.shape[d] > 1 else max(t.stride(d), 1)


class _QueryInitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, flat, K, pos_w, mask):
        B, C, H, W = h.shape
        Ch, dev = flat.shape[1], h.device
        top_class = torch.empty((B, K), dtype=torch.int64, device=dev)
        top_index = torch.empty((B, K), dtype=torch.int64, device=dev)
        query_pos = torch.empty((B, K, 2), dtype=torch.float32, device=dev)
        score = torch.empty((B, C, K), dtype=torch.float32, device=dev)
        rows = torch.empty((B, K, Ch), dtype=flat.dtype, device=dev)
        ws_bytes = _lib.call_size("bfhip_query_init_workspace_bytes", B, C, H, W)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("bfhip_query_init_fwd", h.data_ptr(), _stride(h, 0), _stride(h, 1), _stride(h, 2), _stride(h, 3), B, C, H, W,
                      mask, flat.data_ptr(), flat.stride(0) if B > 1 else 0, flat.stride(2), Ch, _DT[flat.dtype], K, pos_w,
                      top_class.data_ptr(), top_index.data_ptr(), query_pos.data_ptr(), score.data_ptr(), rows.data_ptr(),
                      ws.data_ptr(), ws_bytes, _lib.stream_of(h))
        LAUNCHES["fwd"] += 1
        ctx.mark_non_differentiable(top_class, top_index, query_pos, score)
        ctx.set_materialize_grads(False)   # no zero tensors for the four outputs that carry no gradient
        ctx.save_for_backward(top_index)
        ctx.geom = (B, K, Ch, H * W, flat.dtype)
        return top_class, top_index, query_pos, score, rows

    @staticmethod
    def backward(ctx, _dc, _di, _dp, _ds, d_rows):
        if d_rows is None or not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        (top_index,) = ctx.saved_tensors
        B, K, Ch, HW, dtype = ctx.geom
        if d_rows.dtype != dtype:
            d_rows = d_rows.to(dtype)
        d_rows = d_rows.contiguous()
        if d_rows.data_ptr() % 16:
            d_rows = d_rows.clone()
        d_flat = torch.empty((B, HW, Ch), dtype=dtype, device=d_rows.device)
        with torch.cuda.device(d_rows.device):
            _lib.call("bfhip_query_init_bwd", top_index.data_ptr(), d_rows.data_ptr(), B, K, Ch, HW, _DT[dtype], d_flat.data_ptr(),
                      _lib.stream_of(d_rows))
        LAUNCHES["bwd"] += 1
        return None, d_flat.transpose(1, 2), None, None, None


def fused_query_init(h, flat, K, pos_w, nms_free_classes=()):
    """The HIP path; raises when the call is not supported (no fall-back from here)."""
    if not supported(h, flat, K, 3, nms_free_classes):
        raise RuntimeError("query_init: this call is not covered by csrc/query_init.hip (see query_init.supported)")
    return _QueryInitFn.apply(h, flat, int(K), int(pos_w), class_mask(nms_free_classes, h.shape[1]))


def query_init(h, flat, K, pos_w, nms_free_classes=()):
    """Fused when the tensors are on the device and the kernels cover the call, the torch arithmetic otherwise."""
    if supported(h, flat, K, 3, nms_free_classes):
        return fused_query_init(h, flat, K, pos_w, nms_free_classes)
    return torch_query_init(h, flat, K, pos_w, nms_free_classes)
