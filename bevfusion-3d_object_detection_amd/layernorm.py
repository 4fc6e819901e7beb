"""LayerNorm over the rows of a token matrix with the residual update in front of it (csrc/layernorm.hip).

Three entry points over `[..., C]` tensors viewed as rows, one kernel family behind them:

    layer_norm_rows(x, weight, bias, eps)                          y = LN(x) * weight + bias
    add_layer_norm_rows(x, branch, scale, weight, bias, eps)       s = x + scale[sample] * branch;  y = LN(s) * weight + bias
    scaled_add_rows(x, branch, scale)                              s = x + scale[sample] * branch

`scale` is the per-sample drop-path factor (f32 [B], B = x.shape[0]) or None.  The backward of each is one launch that also adds
the two gradient paths meeting in the residual stream (the gradient of `s` and the one through the norm), which autograd
otherwise does in a kernel of its own; the parameter gradients are per-workgroup partial rows added in a fixed order (no
atomics), and are not computed at all when weight and bias are frozen.

The switch is BFHIP_SWIN_LN (`ENABLED`, read at call time; it ships off, BFHIP_SWIN_LN=1 turns the kernels on).  On the CPU, with
the switch off, or for an input the kernels do not cover (a width that is not a multiple of 8 or exceeds 1536, non-contiguous
rows, no affine parameters, a dtype other than f32 / bf16, unaligned pointers) the functions run the plain torch sequence:
F.layer_norm, multiply, add.
"""
import os

import torch
import torch.nn.functional as F

from . import _lib

ENABLED = os.environ.get("BFHIP_SWIN_LN", "0") != "0"  # ships off until measured: DESIGN.md section 6
LAUNCHES = dict(fwd=0, bwd=0)  # kernel calls made so far (tests and tools read the difference)
_DT = {torch.float32: 0, torch.bfloat16: 1}


def supported(M, C, x_dtype=torch.float32, y_dtype=torch.float32):
    """Host-only: do the kernels cover an [M, C] matrix of these dtypes?"""
    return x_dtype in _DT and y_dtype in _DT and bool(_lib.load().bfhip_layernorm_supported(M, C, _DT[x_dtype], _DT[y_dtype]))


def _dense(t):
    return t.is_cuda and t.is_contiguous() and t.dtype in _DT and t.data_ptr() % 16 == 0


def _affine_ok(weight, bias, C):
    return (weight is not None and bias is not None and weight.dtype == torch.float32 and bias.dtype == torch.float32
            and tuple(weight.shape) == (C,) and tuple(bias.shape) == (C,) and _dense(weight) and _dense(bias))


def _scale_ok(scale, x):
    if scale is None:
        return True
    return (scale.is_cuda and scale.dtype == torch.float32 and scale.dim() == 1 and scale.is_contiguous() and x.dim() >= 2
            and scale.numel() == x.shape[0] and not scale.requires_grad)


def eligible(x, out_dtype, weight=None, bias=None, branch=None, scale=None, affine=True):
    """Does this call run in csrc/layernorm.hip?"""
    if not (ENABLED and x.dim() >= 1 and x.numel() > 0 and _dense(x) and out_dtype in _DT):
        return False
    C = x.shape[-1]
    if affine and not _affine_ok(weight, bias, C):
        return False
    if branch is not None and not (branch.shape == x.shape and _dense(branch) and _scale_ok(scale, x)):
        return False
    return supported(x.numel() // C, C, x.dtype, out_dtype)


def _default_out_dtype(x):
    """What F.layer_norm returns for x: fp32 under autocast (it is on autocast's fp32 list), x's dtype otherwise."""
    return torch.float32 if x.is_cuda and torch.is_autocast_enabled("cuda") else x.dtype


def _run_fwd(x, branch, scale, weight, bias, eps, y_dtype):
    """x, branch [..., C] dense -> (s or None, y or None, mean_rstd or None); y is produced when weight is given."""
    C = x.shape[-1]
    M = x.numel() // C
    s = torch.empty_like(x) if branch is not None else None
    y = stats = None
    if weight is not None:
        y = torch.empty(x.shape, dtype=y_dtype, device=x.device)
        stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    rps = M // scale.numel() if scale is not None else 1
    with torch.cuda.device(x.device):
        _lib.call("bfhip_layernorm_fwd", x.data_ptr(), _lib.ptr(branch), _lib.ptr(scale), rps, _lib.ptr(weight), _lib.ptr(bias), M, C,
                  float(eps), _DT[x.dtype], _DT[branch.dtype] if branch is not None else 0, _DT[y_dtype], _lib.ptr(s), _lib.ptr(y),
                  _lib.ptr(stats), _lib.stream_of(x))
    LAUNCHES["fwd"] += 1
    return s, y, stats


def _run_bwd(s, stats, weight, dy, dsum, scale, x_dtype, branch_dtype, want_dx, want_dbranch, want_affine):
    """One launch (two with the parameter gradients) -> (dx, dbranch, dweight, dbias), None where not wanted."""
    ref = dy if dy is not None else dsum
    C = ref.shape[-1]
    M = ref.numel() // C
    dev = ref.device
    dx = torch.empty(ref.shape, dtype=x_dtype, device=dev) if want_dx else None
    dbranch = torch.empty(ref.shape, dtype=branch_dtype, device=dev) if want_dbranch else None
    partial = dweight = dbias = None
    parts = 0
    if want_affine:
        parts = _lib.load().bfhip_layernorm_parts(M, C)
        partial = torch.empty((parts, 2, C), dtype=torch.float32, device=dev)
        dweight = torch.empty((C,), dtype=torch.float32, device=dev)
        dbias = torch.empty((C,), dtype=torch.float32, device=dev)
    rps = M // scale.numel() if scale is not None else 1
    with torch.cuda.device(dev):
        _lib.call("bfhip_layernorm_bwd", _lib.ptr(s), _lib.ptr(stats), _lib.ptr(weight), _lib.ptr(dy), _lib.ptr(dsum), _lib.ptr(scale),
                  rps, M, C, _DT[x_dtype], _DT[branch_dtype], _DT[dy.dtype] if dy is not None else 0, _lib.ptr(dx),
                  _lib.ptr(dbranch), _lib.ptr(partial), parts, _lib.ptr(dweight), _lib.ptr(dbias), _lib.stream_of(ref))
    LAUNCHES["bwd"] += 1
    return dx, dbranch, dweight, dbias


def _grad_in(g, dtype):
    """An incoming gradient as the dense tensor of `dtype` the kernel reads."""
    if g is None:
        return None
    if g.dtype != dtype:
        g = g.to(dtype)
    g = g.contiguous()
    return g if g.data_ptr() % 16 == 0 else g.clone()


class _NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, y_dtype):
        _, y, stats = _run_fwd(x, None, None, weight, bias, eps, y_dtype)
        ctx.save_for_backward(x, stats, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, stats, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        affine = need[1] or need[2]
        if not (need[0] or affine):
            return None, None, None, None, None
        dx, _, dw, db = _run_bwd(x, stats, weight, _grad_in(dy, dy.dtype), None, None, x.dtype, x.dtype, need[0], False, affine)
        return dx, dw if need[1] else None, db if need[2] else None, None, None


def _add_backward(dsum, scale, branch_dtype, want_dx, want_dbranch):
    """Backward of s = x + scale * branch alone: dx is the incoming gradient itself."""
    dbranch = None
    if want_dbranch:
        if scale is None and dsum.dtype == branch_dtype:
            dbranch = dsum
        else:
            dsum = _grad_in(dsum, dsum.dtype)
            dbranch = _run_bwd(None, None, None, None, dsum, scale, dsum.dtype, branch_dtype, False, True, False)[1]
    return (dsum if want_dx else None), dbranch


class _AddNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, branch, scale, weight, bias, eps, y_dtype):
        s, y, stats = _run_fwd(x, branch, scale, weight, bias, eps, y_dtype)
        ctx.save_for_backward(s, stats, weight, scale)
        ctx.branch_dtype = branch.dtype
        ctx.set_materialize_grads(False)
        return s, y

    @staticmethod
    def backward(ctx, dsum, dy):
        s, stats, weight, scale = ctx.saved_tensors
        need = ctx.needs_input_grad
        affine = (need[3] or need[4]) and dy is not None
        dx = dbranch = dw = db = None
        if dy is None:
            if dsum is not None and (need[0] or need[1]):
                dx, dbranch = _add_backward(dsum, scale, ctx.branch_dtype, need[0], need[1])
        elif need[0] or need[1] or affine:
            dx, dbranch, dw, db = _run_bwd(s, stats, weight, _grad_in(dy, dy.dtype), _grad_in(dsum, s.dtype), scale, s.dtype,
                                           ctx.branch_dtype, need[0], need[1], affine)
        return dx, dbranch, None, dw if need[3] else None, db if need[4] else None, None, None


class _AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, branch, scale):
        s, _, _ = _run_fwd(x, branch, scale, None, None, 0.0, x.dtype)
        ctx.save_for_backward(scale)
        ctx.branch_dtype = branch.dtype
        return s

    @staticmethod
    def backward(ctx, dsum):
        (scale,) = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not (need[0] or need[1]):
            return None, None, None
        dx, dbranch = _add_backward(dsum, scale, ctx.branch_dtype, need[0], need[1])
        return dx, dbranch, None


def _torch_add(x, branch, scale):
    if scale is None:
        return x + branch
    return x + branch * scale.reshape((-1,) + (1,) * (branch.dim() - 1)).to(branch.dtype)


def _torch_norm(x, weight, bias, eps, out_dtype):
    y = F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    return y if out_dtype is None or y.dtype == out_dtype else y.to(out_dtype)


def layer_norm_rows(x, weight, bias, eps=1e-5, out_dtype=None):
    """LayerNorm over the last axis of x [..., C]; `out_dtype` None = what F.layer_norm would return."""
    ydt = out_dtype if out_dtype is not None else _default_out_dtype(x)
    if eligible(x, ydt, weight, bias):
        return _NormFn.apply(x, weight, bias, eps, ydt)
    return _torch_norm(x, weight, bias, eps, out_dtype)


def add_layer_norm_rows(x, branch, scale, weight, bias, eps=1e-5, out_dtype=None):
    """(s, y): s = x + scale[sample] * branch in x's dtype, y = LayerNorm(s).  scale f32 [x.shape[0]] or None."""
    ydt = out_dtype if out_dtype is not None else _default_out_dtype(x)
    if eligible(x, ydt, weight, bias, branch, scale):
        return _AddNormFn.apply(x, branch, scale, weight, bias, eps, ydt)
    s = _torch_add(x, branch, scale)
    return s, _torch_norm(s, weight, bias, eps, out_dtype)


def scaled_add_rows(x, branch, scale=None):
    """s = x + scale[sample] * branch in x's dtype.  scale f32 [x.shape[0]] or None."""
    if eligible(x, x.dtype, branch=branch, scale=scale, affine=False):
        return _AddFn.apply(x, branch, scale)
    return _torch_add(x, branch, scale)
