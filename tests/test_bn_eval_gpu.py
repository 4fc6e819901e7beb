"""GPU: eval-mode BatchNorm (+ residual) (+ ReLU) on the running statistics (csrc/bn_eval.hip) behind bn2d.FUSED_BN_EVAL.

Forward and data gradients are checked element-wise against fp64 computed on the CPU from the stored inputs:
  forward   |got - want| <= [2^-8 |want| for bf16] + 16 * 2^-24 * (|a (x - mean)| + |beta| + |res|)
            (2^-8: bf16's half ulp; the fp32 term covers the rsqrt, one subtract, one fma and one add -- the same formula
            evaluated in fp32 on the CPU needs at most 3.9 of the 16 units)
  dx, dres  |got - want| <= (8 * 2^-24 [+ 2^-8 for bf16]) * |want|, the ReLU mask taken from the kernel's own y
  dgamma, dbeta   max-normalised 1e-4 (f32) / 1.5e-2 (bf16), the bounds of tests/test_bn2d_gpu.py
Stacks are compared with an fp32 twin on the CPU: the kernel path must not be further from it than the torch path."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bevfusion_amd  # noqa: F401
from bevfusion_amd import bn2d, spconv
from bevfusion_amd.dense_modules import SECOND, SECONDFPN, ResNet50

pytestmark = pytest.mark.gpu

EPS = 1e-3
U = 2.0 ** -24
DTYPES = [torch.float32, torch.bfloat16]
COMBOS = [(False, False), (False, True), (True, False), (True, True)]  # (res, relu)
FWD_SHAPES = [(1, 8, 7, 5), (1, 8, 1, 1), (3, 80, 19, 21), (2, 328, 9, 11), (2, 2048, 8, 22), (5, 256, 20, 20)]
BWD_SHAPES = [(3, 80, 19, 21), (2, 328, 9, 11), (1, 8, 7, 5)]
# rows of more than 256 vectors run as column tiles of 256 (the second tile here holds 2 vectors / 1 vector)
TILED = [((2, 1032, 3, 5), torch.float32), ((1, 2056, 3, 5), torch.bfloat16)]
FWD_CASES = [(s, d) for s in FWD_SHAPES for d in DTYPES] + TILED
BWD_CASES = [(s, d) for s in BWD_SHAPES for d in DTYPES] + TILED


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", True)


@functools.lru_cache(maxsize=None)
def case(shape, dtype):
    """CPU inputs of one (shape, dtype) and their fp64 images; shared by the tests, never modified.  shape is (N, C, H, W) or (M, C)."""
    g = torch.Generator().manual_seed(1234 + sum(shape))
    C = shape[1]
    cl = dict(memory_format=torch.channels_last) if len(shape) == 4 else {}
    x = (torch.randn(shape, generator=g) * 1.7 + 0.4).to(dtype).contiguous(**cl)
    res = torch.randn(shape, generator=g).to(dtype).contiguous(**cl)
    dy = torch.randn(shape, generator=g).to(dtype).contiguous(**cl)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.rand(C, generator=g) - 0.5
    mean = torch.randn(C, generator=g)
    var = torch.rand(C, generator=g) * 1.5 + 0.5
    v = (1, C) + (1,) * (len(shape) - 2)
    rstd = 1.0 / torch.sqrt(var.double() + EPS)
    xhat = (x.double() - mean.double().view(v)) * rstd.view(v)
    z = xhat * gamma.double().view(v)
    return dict(x=x, res=res, dy=dy, gamma=gamma, beta=beta, mean=mean, var=var, view=v, xhat=xhat, z=z,
                a=(gamma.double() * rstd).view(v))


def module(cls, c, dev, **kw):
    m = cls(c["gamma"].numel(), eps=EPS, **kw).to(dev)
    with torch.no_grad():
        m.weight.copy_(c["gamma"])
        m.bias.copy_(c["beta"])
        m.running_mean.copy_(c["mean"])
        m.running_var.copy_(c["var"])
    return m.eval()


def check_forward(c, got, res, relu, dtype):
    want = c["z"] + c["beta"].double().view(c["view"])
    mag = c["z"].abs() + c["beta"].double().abs().view(c["view"])
    if res:
        want = want + c["res"].double()
        mag = mag + c["res"].double().abs()
    if relu:
        want = want.clamp(min=0)
    bound = 16 * U * mag
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * want.abs()
    err = (got.detach().cpu().double() - want).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print("forward: worst error / bound = %.3f" % worst)
    assert bool((err <= bound).all()), worst


def buffers(m):
    return [m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()]


@pytest.mark.parametrize("res,relu", COMBOS)
@pytest.mark.parametrize("shape,dtype", FWD_CASES)
def test_forward_against_fp64(dev, on, shape, dtype, res, relu):
    c = case(shape, dtype)
    bn = module(bn2d.BatchNorm2dAct, c, dev)
    x = c["x"].to(dev)
    r = c["res"].to(dev) if res else None
    assert bn.eval_fusable(x)
    before, launches = buffers(bn), dict(bn2d.EVAL_LAUNCHES)
    with torch.no_grad():
        y = bn(x, residual=r, relu=relu)
    assert bn2d.EVAL_LAUNCHES["fwd"] == launches["fwd"] + 1 and bn2d.EVAL_LAUNCHES["bwd"] == launches["bwd"]
    assert y.dtype == dtype and y.shape == x.shape and y.is_contiguous(memory_format=torch.channels_last)
    for u, v in zip(before, buffers(bn)):
        assert torch.equal(u, v)
    check_forward(c, y, res, relu, dtype)


def torch_path(bn, x, r, relu):
    out = F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
    if r is not None:
        out = out + r
    return F.relu(out) if relu else out


def test_fallbacks_are_the_torch_expression(dev, monkeypatch):
    c = case((3, 80, 19, 21), torch.float32)
    launches = dict(bn2d.EVAL_LAUNCHES)
    with torch.no_grad():
        # the flag off
        monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", False)
        bn = module(bn2d.BatchNorm2dAct, c, dev)
        x, r = c["x"].to(dev), c["res"].to(dev)
        assert not bn.eval_fusable(x)
        assert torch.equal(bn(x, residual=r, relu=True), torch_path(bn, x, r, True))
        monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", True)
        assert bn.eval_fusable(x)
        # NCHW-contiguous input
        xc = x.contiguous()
        assert not bn.eval_fusable(xc)
        assert torch.equal(bn(xc, residual=r, relu=True), torch_path(bn, xc, r, True))
        # training mode is not this path's business
        assert not bn.train().eval_fusable(x)
        bn.eval()
        # 6 channels: not a multiple of the 16-byte vector
        bn6 = bn2d.BatchNorm2dAct(6, eps=EPS).to(dev).eval()
        bn6.running_mean.normal_()
        bn6.running_var.uniform_(0.5, 2.0)
        x6 = torch.randn(2, 6, 5, 5, device=dev).contiguous(memory_format=torch.channels_last)
        assert not bn6.eval_fusable(x6)
        assert torch.equal(bn6(x6, relu=True), torch_path(bn6, x6, None, True))
        # the CPU
        cpu = module(bn2d.BatchNorm2dAct, c, "cpu")
        assert not cpu.eval_fusable(c["x"])
        assert torch.equal(cpu(c["x"], residual=c["res"], relu=True), torch_path(cpu, c["x"], c["res"], True))
    assert bn2d.EVAL_LAUNCHES == launches


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30))


@pytest.mark.parametrize("res,relu", COMBOS)
@pytest.mark.parametrize("shape,dtype", BWD_CASES)
def test_backward_against_fp64(dev, on, shape, dtype, res, relu):
    c = case(shape, dtype)
    bn = module(bn2d.BatchNorm2dAct, c, dev)
    x = c["x"].to(dev).requires_grad_(True)
    r = c["res"].to(dev).requires_grad_(True) if res else None
    dy = c["dy"].to(dev)
    launches = dict(bn2d.EVAL_LAUNCHES)
    y = bn(x, residual=r, relu=relu)
    ins = [x, bn.weight, bn.bias] + ([r] if res else [])
    grads = torch.autograd.grad(y, ins, dy, retain_graph=True)
    again = torch.autograd.grad(y, ins, dy)
    assert bn2d.EVAL_LAUNCHES == dict(fwd=launches["fwd"] + 1, bwd=launches["bwd"] + 2)
    assert torch.equal(grads[1], again[1]) and torch.equal(grads[2], again[2])  # fixed summation order
    g = c["dy"].double()
    if relu:
        g = g * (y.detach().cpu() > 0)
    tol = 8 * U + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    ptol = 1e-4 if dtype == torch.float32 else 1.5e-2

    def elementwise(got, want, what):
        assert got.dtype == dtype and got.shape == want.shape
        err, bound = (got.cpu().double() - want).abs(), tol * want.abs()
        worst = float((err / bound.clamp(min=1e-300)).max())
        print("%s: worst error / bound = %.3f" % (what, worst))
        assert bool((err <= bound).all()), (what, worst)

    elementwise(grads[0], g * c["a"], "dx")
    if res:
        elementwise(grads[3], g, "dres")
    dims = [d for d in range(len(shape)) if d != 1]
    e_g, e_b = rel(grads[1].cpu(), (g * c["xhat"]).sum(dims)), rel(grads[2].cpu(), g.sum(dims))
    print("dgamma %.3g dbeta %.3g (bound %g)" % (e_g, e_b, ptol))
    assert e_g <= ptol and e_b <= ptol


@pytest.mark.parametrize("relu", [False, True])
def test_backward_with_frozen_affine_needs_no_partial_buffer(dev, on, monkeypatch, relu):
    c = case((3, 80, 19, 21), torch.bfloat16)
    bn = module(bn2d.BatchNorm2dAct, c, dev).requires_grad_(False)
    x = c["x"].to(dev).requires_grad_(True)
    r = c["res"].to(dev).requires_grad_(True)
    calls = []
    real = bn2d._lib.call

    def spy(name, *args):
        calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(bn2d._lib, "call", spy)
    launches = dict(bn2d.EVAL_LAUNCHES)
    y = bn(x, residual=r, relu=relu)
    y.backward(c["dy"].to(dev))
    assert bn2d.EVAL_LAUNCHES == dict(fwd=launches["fwd"] + 1, bwd=launches["bwd"] + 1)
    (args,) = [a for n, a in calls if n == "bfhip_bn_eval_bwd"]
    assert args[2] is None and args[13] is None and args[14] is None  # x, partial, dgb
    assert (args[1] is None) == (not relu)                             # y only with ReLU
    assert bn.weight.grad is None and bn.bias.grad is None
    g = c["dy"].double() * ((y.detach().cpu() > 0) if relu else 1)
    assert torch.equal(r.grad.cpu().double(), g)
    assert rel(x.grad.cpu(), g * c["a"]) <= 2.0 ** -8


ROW_SHAPES = [((1000, 16), torch.float32), ((1000, 128), torch.float32), ((1000, 48), torch.float32), ((999, 64), torch.bfloat16)]


@pytest.mark.parametrize("shape,dtype", ROW_SHAPES)
def test_rows_modules_in_eval(dev, on, shape, dtype):
    c = case(shape, dtype)
    x, r = c["x"].to(dev), c["res"].to(dev)
    rows = module(bn2d.BatchNormRows, c, dev)
    sp = module(spconv.BatchNorm1dAct, c, dev)
    assert rows.eval_fusable(x)
    launches = dict(bn2d.EVAL_LAUNCHES)
    with torch.no_grad():
        for relu in (False, True):
            y = rows(x, relu=relu)
            assert y.dtype == dtype and y.shape == x.shape and y.is_contiguous()
            check_forward(c, y, False, relu, dtype)
        for res, relu in COMBOS:
            y = sp(x, residual=r if res else None, relu=relu)
            assert y.dtype == dtype and y.shape == x.shape and y.is_contiguous()
            check_forward(c, y, res, relu, dtype)
        with pytest.raises(RuntimeError):
            sp(x, rows_dev=torch.tensor([shape[0]], dtype=torch.int32, device=dev))  # static capacity stays training-only
    assert bn2d.EVAL_LAUNCHES["fwd"] == launches["fwd"] + 6


# ----------------------------------------------------------------------------- stacks against an fp32 twin on the CPU
def l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


def randomise_running_stats(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.modules.batchnorm._BatchNorm):
                m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))


class BevStack(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = SECOND(256, [128, 256], [5, 5], [1, 2])
        self.neck = SECONDFPN([128, 256], [256, 256], [1, 2], use_conv_for_no_stride=True)

    def forward(self, x):
        return self.neck(self.backbone(x))[0]


@pytest.fixture(scope="module")
def bev_stack():
    torch.manual_seed(0)
    twin = BevStack()
    randomise_running_stats(twin, 5)
    twin.eval()
    x = torch.randn(2, 256, 64, 64, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        want = twin(x)
    return twin, x, want


def run_bev(twin, x, dev, flag, monkeypatch, autocast):
    monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", flag)
    net = copy.deepcopy(twin).to(dev).eval()
    before = bn2d.EVAL_LAUNCHES["fwd"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = net(x.to(dev).contiguous(memory_format=torch.channels_last))
    return y, bn2d.EVAL_LAUNCHES["fwd"] - before


def test_second_stack_fp32(dev, bev_stack, monkeypatch):
    twin, x, want = bev_stack
    y, n = run_bev(twin, x, dev, True, monkeypatch, False)
    e = l2(y, want)
    print("fp32 SECOND + SECONDFPN: relative L2 %.3g, %d kernel forwards" % (e, n))
    assert n == 14  # 12 BatchNorms in SECOND, 2 in SECONDFPN
    assert y.dtype == torch.float32 and e <= 1e-4


def test_second_stack_bf16_is_no_worse_than_the_torch_path(dev, bev_stack, monkeypatch):
    twin, x, want = bev_stack
    y_on, n_on = run_bev(twin, x, dev, True, monkeypatch, True)
    y_off, n_off = run_bev(twin, x, dev, False, monkeypatch, True)
    e_on, e_off = l2(y_on, want), l2(y_off, want)
    print("bf16 SECOND + SECONDFPN: e_on %.3g e_off %.3g" % (e_on, e_off))
    assert (n_on, n_off) == (14, 0)
    assert e_on <= 1.25 * e_off + 1e-3 and e_on <= 1e-2


RESNET_GRADS = ("layer2.0.conv1.weight", "layer4.2.bn3.weight")
RESNET_FROZEN = ("conv1.", "bn1.", "layer1.")


def resnet_step(net, x, autocast):
    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        outs = net(x)
    sum(o.float().square().mean() for o in outs).backward()
    params = dict(net.named_parameters())
    return [o.detach().float().cpu() for o in outs] + [params[n].grad.detach().float().cpu() for n in RESNET_GRADS]


def test_resnet_norm_eval_training_step(dev, monkeypatch):
    torch.manual_seed(0)
    twin = ResNet50(norm_eval=True, frozen_stages=1)
    randomise_running_stats(twin, 7)
    twin.train()
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(8))
    net = copy.deepcopy(twin).to(dev).train()
    want = resnet_step(twin, x, False)
    monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", True)
    launches = dict(bn2d.EVAL_LAUNCHES)
    got_on = resnet_step(net, x.to(dev), True)
    assert bn2d.EVAL_LAUNCHES["fwd"] == launches["fwd"] + 53  # the stem, 16 x 3 in the bottlenecks, 4 shortcuts
    assert bn2d.EVAL_LAUNCHES["bwd"] > launches["bwd"]
    for n, p in net.named_parameters():
        if n.startswith(RESNET_FROZEN):
            assert p.grad is None, n
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    monkeypatch.setattr(bn2d, "FUSED_BN_EVAL", False)
    got_off = resnet_step(net, x.to(dev), True)
    assert bn2d.EVAL_LAUNCHES["fwd"] == launches["fwd"] + 53
    for name, a, b, w in zip(("out0", "out1", "out2") + RESNET_GRADS, got_on, got_off, want):
        e_on, e_off = l2(a, w), l2(b, w)
        print("%s: e_on %.3g e_off %.3g" % (name, e_on, e_off))
        assert e_on <= 1.25 * e_off + 1e-3, name


def test_training_mode_does_not_touch_the_eval_kernels(dev, on):
    torch.manual_seed(0)
    net = SECOND(256, [128, 256], [1, 1], [1, 2]).to(dev).train()
    x = torch.randn(2, 256, 32, 32, device=dev).contiguous(memory_format=torch.channels_last)
    launches = dict(bn2d.EVAL_LAUNCHES)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        outs = net(x)
    sum(o.float().square().mean() for o in outs).backward()
    assert net.blocks[0][0].weight.grad is not None
    assert bn2d.EVAL_LAUNCHES == launches
