"""GPU: eval-mode BatchNorm over a capacity-sized [M, C] matrix whose active rows are a prefix counted on the device
(bfhip_bn_eval_rows_fwd / _bwd in csrc/bn_eval.hip), and spconv.BatchNorm1dAct on top of it.

With n = min(max(*rows_dev, 0), M): the rows below n carry the bits of bfhip_bn_eval_fwd / _bwd run on the contiguous [n, C]
slice, the rows from n on are exactly zero whatever the inputs hold there (NaN and 1e30 here), and dgamma / dbeta carry the
bits of bfhip_bn_eval_bwd on the whole matrix with dy zeroed and x made finite beyond n (same partition of the rows, the masked
rows add exact zeros).  Through the module the kernel path is checked against fp64 with the forward bound of
tests/test_bn_eval_gpu.py, 16 * 2^-24 * (|a (x - mean)| + |beta| + |res|) [+ 2^-8 |want| for bf16], and the torch fallback
(BFHIP_BN_EVAL=0) against the kernel path with that file's kernel-vs-torch bounds (relative L2 1e-4 fp32, 1e-2 bf16)."""
import functools

import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, bn2d, spconv

pytestmark = pytest.mark.gpu

EPS = 1e-3
U = 2.0 ** -24
DT = {torch.float32: 0, torch.bfloat16: 1}
COMBOS = [(False, False), (False, True), (True, False), (True, True)]  # (res, relu)
ROWS = {1000: (0, 1, 63, 64, 65, 999, 1000, 1500, -3), 1: (0, 1, 1500, -3)}  # capacity -> counts (1500, -3: clamped)
CASES = [(C, dt) for C in (16, 128) for dt in (torch.float32, torch.bfloat16)]


@functools.lru_cache(maxsize=None)
def case(M, C, dtype):
    """CPU inputs of one shape; shared by the tests, never modified."""
    g = torch.Generator().manual_seed(77 + M + C)
    mk = lambda s, o: (torch.randn(M, C, generator=g) * s + o).to(dtype)  # noqa: E731
    return dict(x=mk(1.7, 0.4), res=mk(1.0, 0.0), dy=mk(1.0, 0.0), gamma=torch.rand(C, generator=g) + 0.5,
                beta=torch.rand(C, generator=g) - 0.5, mean=torch.randn(C, generator=g), var=torch.rand(C, generator=g) * 1.5 + 0.5)


def poisoned(t, n):
    """t with its rows from n on holding NaN and +-1e30 in turn"""
    t = t.clone()
    if n < t.shape[0]:
        tail = torch.full_like(t[n:], float("nan"))
        tail[:, 1::3] = 1e30
        tail[:, 2::3] = -1e30
        t[n:] = tail
    return t


def on_dev(c, dev):
    return {k: v.to(dev) for k, v in c.items()}


def fwd(d, x, res, M, C, relu, rows=None):
    y = torch.full_like(x[:M], 7.0)
    head = (x.data_ptr(), _lib.ptr(res), d["gamma"].data_ptr(), d["beta"].data_ptr(), d["mean"].data_ptr(), d["var"].data_ptr(),
            M, C, DT[x.dtype], EPS, 1 if relu else 0, y.data_ptr())
    if rows is None:
        _lib.call("bfhip_bn_eval_fwd", *head, _lib.stream_of(x))
    else:
        _lib.call("bfhip_bn_eval_rows_fwd", *head, rows.data_ptr(), _lib.stream_of(x))
    return y


def bwd(d, dy, y, x, M, C, relu, rows=None):
    """-> dx, dres, dgb (all three requested)"""
    dx, dres = torch.full_like(dy[:M], 7.0), torch.full_like(dy[:M], 7.0)
    parts = _lib.load().bfhip_bn_eval_parts(M, C, DT[dy.dtype])
    partial = torch.empty(parts, 2, C, dtype=torch.float32, device=dy.device)
    dgb = torch.full((2 * C,), 7.0, dtype=torch.float32, device=dy.device)
    head = (dy.data_ptr(), _lib.ptr(y) if relu else None, x.data_ptr(), d["gamma"].data_ptr(), d["mean"].data_ptr(),
            d["var"].data_ptr(), M, C, DT[dy.dtype], EPS, 1 if relu else 0, dx.data_ptr(), dres.data_ptr(), partial.data_ptr(),
            dgb.data_ptr())
    if rows is None:
        _lib.call("bfhip_bn_eval_bwd", *head, _lib.stream_of(dy))
    else:
        _lib.call("bfhip_bn_eval_rows_bwd", *head, rows.data_ptr(), _lib.stream_of(dy))
    return dx, dres, dgb


def zero(t):
    return bool((t == 0).all())


@pytest.mark.parametrize("M", sorted(ROWS))
@pytest.mark.parametrize("C,dtype", CASES)
def test_forward_prefix_bits_and_zero_tail(dev, C, dtype, M):
    d = on_dev(case(M, C, dtype), dev)
    assert _lib.load().bfhip_bn_eval_supported(M, C, DT[dtype]) == 1
    for count in ROWS[M]:
        n = min(max(count, 0), M)
        rows = torch.tensor([count], dtype=torch.int32, device=dev)
        x, r = poisoned(d["x"], n), poisoned(d["res"], n)
        for res, relu in COMBOS:
            y = fwd(d, x, r if res else None, M, C, relu, rows)
            assert zero(y[n:]), (count, res, relu)
            if n:
                want = fwd(d, x[:n], r[:n] if res else None, n, C, relu)
                assert torch.equal(y[:n], want), (count, res, relu)
            assert torch.equal(y, fwd(d, x, r if res else None, M, C, relu, rows))  # run to run


@pytest.mark.parametrize("M", sorted(ROWS))
@pytest.mark.parametrize("C,dtype", CASES)
def test_backward_prefix_bits_zero_tail_and_parameter_sums(dev, C, dtype, M):
    d = on_dev(case(M, C, dtype), dev)
    for count in ROWS[M]:
        n = min(max(count, 0), M)
        rows = torch.tensor([count], dtype=torch.int32, device=dev)
        x, dy = poisoned(d["x"], n), poisoned(d["dy"], n)
        x_fin, dy_zero = d["x"].clone(), d["dy"].clone()
        x_fin[n:] = 1.0
        dy_zero[n:] = 0
        for res, relu in COMBOS:
            y_full = fwd(d, d["x"], d["res"] if res else None, M, C, relu)  # the ReLU mask of the active rows
            y = poisoned(y_full, n)
            dx, dres, dgb = bwd(d, dy, y, x, M, C, relu, rows)
            assert zero(dx[n:]) and zero(dres[n:]), (count, res, relu)
            if n:
                wdx, wdres, _ = bwd(d, dy[:n], y[:n], x[:n], n, C, relu)
                assert torch.equal(dx[:n], wdx) and torch.equal(dres[:n], wdres), (count, res, relu)
            _, _, wdgb = bwd(d, dy_zero, y_full, x_fin, M, C, relu)
            assert torch.equal(dgb, wdgb), (count, res, relu)
            again = bwd(d, dy, y, x, M, C, relu, rows)
            assert all(torch.equal(a, b) for a, b in zip((dx, dres, dgb), again))


# kernel path against torch path in tests/test_bn_eval_gpu.py: relative L2 of 1e-4 for fp32 and 1e-2 for bf16 (its two stack
# tests).  The element-wise fp64 bound above is the KERNEL's (one rounding at the store); the torch expression rounds after the
# affine map, after the residual add and after the ReLU, which in bf16 is up to three half-ulps
STACK_L2 = {torch.float32: 1e-4, torch.bfloat16: 1e-2}


def l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


def module(c, dev, C):
    m = spconv.BatchNorm1dAct(C, eps=EPS).to(dev)
    with torch.no_grad():
        m.weight.copy_(c["gamma"])
        m.bias.copy_(c["beta"])
        m.running_mean.copy_(c["mean"])
        m.running_var.copy_(c["var"])
    return m.eval()


def fp64_forward(c, res, relu):
    a = c["gamma"].double() / torch.sqrt(c["var"].double() + EPS)
    z = (c["x"].double() - c["mean"].double()) * a
    want, mag = z + c["beta"].double(), z.abs() + c["beta"].double().abs()
    if res:
        want, mag = want + c["res"].double(), mag + c["res"].double().abs()
    return (want.clamp(min=0) if relu else want), mag


@pytest.mark.parametrize("C,dtype", CASES)
def test_module_in_eval_kernel_and_torch_fallback(dev, monkeypatch, C, dtype):
    """BatchNorm1dAct(rows_dev=) in eval once its owner has opted in (static_eval): the kernels when bn2d._eval_fusable holds,
    the sync-free torch expression otherwise (BFHIP_BN_EVAL=0, unsupported width); without the opt-in the call raises as before."""
    M, n = 1000, 637
    c = case(M, C, dtype)
    d = on_dev(c, dev)
    bn = module(c, dev, C)
    rows = torch.tensor([n], dtype=torch.int32, device=dev)
    x, r = poisoned(d["x"], n), poisoned(d["res"], n)
    with pytest.raises(RuntimeError):
        bn(x, rows_dev=rows)
    bn.static_eval = True
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = {}
        for flag in (True, False):
            monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", flag)
            before = bn2d.EVAL_LAUNCHES["fwd"]
            with torch.no_grad():
                out[flag] = [bn(x, residual=r if res else None, relu=relu, rows_dev=rows) for res, relu in COMBOS]
            assert bn2d.EVAL_LAUNCHES["fwd"] - before == (4 if flag else 0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k, (res, relu) in enumerate(COMBOS):
        want, mag = fp64_forward(c, res, relu)
        bound = 16 * U * mag + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0.0)
        for flag in (True, False):
            y = out[flag][k]
            assert y.dtype == dtype and y.shape == (M, C) and zero(y[n:]), (flag, res, relu)
        err = (out[True][k][:n].cpu().double() - want[:n]).abs()
        worst = float((err / bound[:n].clamp(min=1e-300)).max())
        e = l2(out[False][k][:n], out[True][k][:n])
        print("res=%s relu=%s: kernel worst error / bound = %.3f, torch fallback vs kernel relative L2 %.3g" % (res, relu, worst, e))
        assert bool((err <= bound[:n]).all()), (res, relu, worst)
        assert e <= STACK_L2[dtype], (res, relu, e)
        assert torch.equal(out[True][k], fwd(d, x, r if res else None, M, C, relu, rows))
    # a width the kernels do not take (6 channels): the torch expression, same masking
    bn6 = spconv.BatchNorm1dAct(6, eps=EPS).to(dev).eval()
    bn6.static_eval = True
    monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", True)
    x6 = poisoned(torch.randn(50, 6, device=dev), 20)
    y6 = bn6(x6, relu=True, rows_dev=torch.tensor([20], dtype=torch.int32, device=dev))
    assert zero(y6[20:]) and torch.equal(y6[:20], torch.relu(torch.nn.functional.batch_norm(
        x6[:20], bn6.running_mean, bn6.running_var, bn6.weight, bn6.bias, False, 0.0, EPS)))


@pytest.mark.parametrize("fused", [True, False])
def test_module_backward_masks_the_padding(dev, monkeypatch, fused):
    """autograd through the eval module with rows_dev: gradients of x and the residual are zero beyond the count, and the
    parameter gradients are those of the active rows alone (the kernels against the torch expression, bounds of test_bn_eval_gpu)."""
    M, C, n = 1000, 128, 637
    c = case(M, C, torch.float32)
    d = on_dev(c, dev)
    rows = torch.tensor([n], dtype=torch.int32, device=dev)
    monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", fused)
    bn = module(c, dev, C)
    bn.static_eval = True
    x = poisoned(d["x"], n).requires_grad_(True)
    r = poisoned(d["res"], n).requires_grad_(True)
    before = bn2d.EVAL_LAUNCHES["bwd"]
    y = bn(x, residual=r, relu=True, rows_dev=rows)
    dy = d["dy"].clone()
    y.backward(dy)
    assert bn2d.EVAL_LAUNCHES["bwd"] - before == (1 if fused else 0)
    assert zero(x.grad[n:]) and zero(r.grad[n:])
    ref = module(c, dev, C)
    monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", False)
    xs, rs = d["x"][:n].clone().requires_grad_(True), d["res"][:n].clone().requires_grad_(True)
    ref(xs, residual=rs, relu=True).backward(dy[:n])
    tol = 8 * U
    for got, want in ((x.grad[:n], xs.grad), (r.grad[:n], rs.grad)):
        assert bool(((got - want).abs() <= tol * want.abs()).all())
    for got, want in ((bn.weight.grad, ref.weight.grad), (bn.bias.grad, ref.bias.grad)):
        assert float((got - want).abs().max() / want.abs().max()) <= 1e-4
