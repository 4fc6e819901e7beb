"""GPU: row LayerNorm with the residual update in front of it (csrc/layernorm.hip, bevfusion_amd/layernorm.py) against torch in
fp64 on the CPU, computed from the same stored inputs, and the Swin block with the kernels on against the same block with them
off.

Tolerances are the project's own for fused BatchNorm (tests/test_bn2d_gpu.py::test_bn2d_matches_torch): max-norm ratio
tests/util.rel_err < 1e-4 for f32 outputs, < 1.5e-2 for bf16 outputs.  A bf16 y is also held element by element to
|got - want| <= 2^-8 |want| + 1e-6: one bf16 rounding is 2^-9, and an fp32-level difference in front of it may flip the
rounding, which costs up to one ulp.  The block comparison uses the 3e-2 of tests/test_swin_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, layernorm, swin
from test_swin_cpu import rel
from util import rel_err

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-5
WIDTHS = [96, 192, 384, 768, 1536]


@pytest.fixture(autouse=True)
def kernels_on(monkeypatch):
    """The tests here are about the kernel path whatever default BFHIP_SWIN_LN ships with (tests that want it off say so)."""
    monkeypatch.setattr(layernorm, "ENABLED", True)


def tol(dtype):
    return 1e-4 if dtype == F32 else 1.5e-2


def check(name, got, want, dtype=None):
    dtype = dtype or got.dtype
    assert got.dtype == dtype, (name, got.dtype)
    e = rel_err(got.detach().double().cpu().numpy(), want.detach().numpy())
    print("%s %s %.2e" % (name, str(dtype).replace("torch.", ""), e))
    assert e < tol(dtype), (name, e)


def check_bf16_elementwise(name, got, want):
    got, want = got.detach().double().cpu(), want.detach()
    worst = float(((got - want).abs() - (2.0 ** -8 * want.abs() + 1e-6)).max())
    print("%s element-wise slack %.2e" % (name, -worst))
    assert worst <= 0, (name, worst)


def params(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    w = (1.0 + 0.5 * torch.randn(C, generator=g)).to(dev)
    b = (0.3 * torch.randn(C, generator=g)).to(dev)
    return w, b


def ref_norm(s, w, b):
    """fp64 LayerNorm (biased variance) -> y, mean, rstd"""
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return (s - mean) * rstd * w + b, mean.squeeze(-1), rstd.squeeze(-1)


# ------------------------------------------------------------------------------------------------ 1. norm mode
@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (F32, BF16), (BF16, BF16)], ids=["f32-f32", "f32-bf16", "bf16-bf16"])
@pytest.mark.parametrize("M", [1, 37, 4099])
@pytest.mark.parametrize("C", WIDTHS)
def test_norm_forward_backward(dev, C, M, xdt, ydt):
    """Row tail (M = 1, 37), workgroup tail and more than one partial row (4099); mean 3, std 2 so that a one-pass variance shows."""
    g = torch.Generator().manual_seed(C + M)
    x = (3.0 + 2.0 * torch.randn(M, C, generator=g)).to(xdt).to(dev).requires_grad_(True)
    dy = torch.randn(M, C, generator=g).to(ydt).to(dev)
    w, b = params(C, dev, 1)
    w.requires_grad_(True), b.requires_grad_(True)
    assert layernorm.eligible(x, ydt, w, b)
    before = dict(layernorm.LAUNCHES)
    y = layernorm.layer_norm_rows(x, w, b, EPS, ydt)
    assert layernorm.LAUNCHES["fwd"] == before["fwd"] + 1
    dx, dw, db = torch.autograd.grad(y, [x, w, b], dy)
    assert layernorm.LAUNCHES["bwd"] == before["bwd"] + 1
    stats = layernorm._run_fwd(x.detach(), None, None, w.detach(), b.detach(), EPS, ydt)[2]

    xr = x.detach().double().cpu().requires_grad_(True)
    wr, br = w.detach().double().cpu().requires_grad_(True), b.detach().double().cpu().requires_grad_(True)
    yr, mean, rstd = ref_norm(xr, wr, br)
    dxr, dwr, dbr = torch.autograd.grad(yr, [xr, wr, br], dy.double().cpu())
    check("y", y, yr, ydt)
    if ydt == BF16:
        check_bf16_elementwise("y", y, yr)
    check("mean", stats[:, 0], mean, F32)
    check("rstd", stats[:, 1], rstd, F32)
    check("dx", dx, dxr, xdt)
    check("dgamma", dw, dwr, F32)
    check("dbeta", db, dbr, F32)
    assert layernorm._lib.load().bfhip_layernorm_parts(M, C) > (1 if M == 4099 else 0)


# ------------------------------------------------------------------------------------------------ 2. add + norm, add
def _add_case(C, dev, with_scale, B=3, rows=35, seed=0, xdt=F32, bdt=BF16, ydt=BF16):
    g = torch.Generator().manual_seed(seed + C)
    t = dict(x=(3.0 + 2.0 * torch.randn(B, rows, C, generator=g)).to(xdt), branch=(1.5 * torch.randn(B, rows, C, generator=g)).to(bdt),
             dsum=torch.randn(B, rows, C, generator=g).to(xdt), dy=torch.randn(B, rows, C, generator=g).to(ydt))
    scale = None
    if with_scale:
        scale = (torch.rand(B, generator=g) < 0.7).float() / 0.8 if B > 3 else torch.tensor([0.0, 1 / 0.8, 1 / 0.8][:B])
    return t, scale


def _ref_add(t, scale):
    xr, br = t["x"].double().requires_grad_(True), t["branch"].double().requires_grad_(True)
    sr = xr + (br if scale is None else br * scale.double().view(-1, 1, 1))
    return xr, br, sr


@pytest.mark.parametrize("with_scale", [True, False], ids=["scale", "noscale"])
@pytest.mark.parametrize("C", [96, 384])
def test_add_norm(dev, C, with_scale):
    """3 samples of 35 rows: sample boundaries fall inside a workgroup.  f32 stream, bf16 branch and y, dsum and dy both non-zero."""
    t, scale = _add_case(C, dev, with_scale)
    x, branch = t["x"].to(dev).requires_grad_(True), t["branch"].to(dev).requires_grad_(True)
    w, b = params(C, dev, 2)
    w.requires_grad_(True), b.requires_grad_(True)
    sc = scale.to(dev) if with_scale else None
    assert layernorm.eligible(x, BF16, w, b, branch, sc)
    before = dict(layernorm.LAUNCHES)
    s, y = layernorm.add_layer_norm_rows(x, branch, sc, w, b, EPS, BF16)
    dx, dbranch, dw, db = torch.autograd.grad([s, y], [x, branch, w, b], [t["dsum"].to(dev), t["dy"].to(dev)])
    assert (layernorm.LAUNCHES["fwd"], layernorm.LAUNCHES["bwd"]) == (before["fwd"] + 1, before["bwd"] + 1)

    xr, br, sr = _ref_add(t, scale)
    wr, bb = w.detach().double().cpu().requires_grad_(True), b.detach().double().cpu().requires_grad_(True)
    yr = ref_norm(sr, wr, bb)[0]
    dxr, dbrr, dwr, dbr = torch.autograd.grad([sr, yr], [xr, br, wr, bb], [t["dsum"].double(), t["dy"].double()])
    check("s", s, sr, F32)
    check("y", y, yr, BF16)
    check_bf16_elementwise("y", y, yr)
    check("dx", dx, dxr, F32)
    check("dbranch", dbranch, dbrr, BF16)
    check("dgamma", dw, dwr, F32)
    check("dbeta", db, dbr, F32)
    if with_scale:  # the dropped sample: no gradient into its branch, and the stream gradient is still dsum + dLN
        assert bool((dbranch[0] == 0).all())
        assert torch.equal(s[0], x[0].detach())
        yr0 = ref_norm(xr[0], wr, bb)[0]
        dln0 = torch.autograd.grad(yr0, xr, t["dy"][0].double())[0][0]
        check("dx[dropped]", dx[0], t["dsum"][0].double() + dln0, F32)


@pytest.mark.parametrize("with_scale", [True, False], ids=["scale", "noscale"])
@pytest.mark.parametrize("C", [96, 384])
def test_add_only(dev, C, with_scale):
    t, scale = _add_case(C, dev, with_scale, seed=5)
    x, branch = t["x"].to(dev).requires_grad_(True), t["branch"].to(dev).requires_grad_(True)
    sc = scale.to(dev) if with_scale else None
    before = dict(layernorm.LAUNCHES)
    s = layernorm.scaled_add_rows(x, branch, sc)
    assert layernorm.LAUNCHES["fwd"] == before["fwd"] + 1
    dsum = t["dsum"].to(dev)
    dx, dbranch = torch.autograd.grad(s, [x, branch], dsum)
    xr, br, sr = _ref_add(t, scale)
    dxr, dbrr = torch.autograd.grad(sr, [xr, br], t["dsum"].double())
    check("s", s, sr, F32)
    assert torch.equal(dx, dsum)
    check("dbranch", dbranch, dbrr, BF16)
    if with_scale:
        assert bool((dbranch[0] == 0).all())


def test_add_norm_bf16_stream(dev):
    """A bf16 stream: s is rounded to bf16 when stored, and y normalises that stored value."""
    C = 192
    t, scale = _add_case(C, dev, True, seed=9, xdt=BF16)
    x, branch, sc = t["x"].to(dev).requires_grad_(True), t["branch"].to(dev).requires_grad_(True), scale.to(dev)
    w, b = params(C, dev, 3)
    s, y = layernorm.add_layer_norm_rows(x, branch, sc, w, b, EPS, BF16)
    xr, br, sr = _ref_add(t, scale)
    check("s", s, sr, BF16)
    stored = s.detach().double().cpu().requires_grad_(True)
    yr = ref_norm(stored, w.double().cpu(), b.double().cpu())[0]
    check("y", y, yr, BF16)
    check_bf16_elementwise("y", y, yr)
    dx, dbranch = torch.autograd.grad([s, y], [x, branch], [t["dsum"].to(dev), t["dy"].to(dev)])
    dsr = torch.autograd.grad(yr, stored, t["dy"].double())[0] + t["dsum"].double()
    check("dx", dx, dsr, BF16)
    check("dbranch", dbranch, dsr * scale.double().view(-1, 1, 1), BF16)


# ------------------------------------------------------------------------------------------------ 3. reproducibility
def test_backward_is_reproducible(dev):
    """4099 samples of one row each (a per-row drop-path factor), several partial rows: two runs agree bit for bit."""
    C = 96
    t, scale = _add_case(C, dev, True, B=4099, rows=1, seed=11)
    assert 0 < int((scale == 0).sum()) < 4099
    w, b = params(C, dev, 4)
    w.requires_grad_(True), b.requires_grad_(True)
    assert _lib.load().bfhip_layernorm_parts(4099, C) > 1
    runs = []
    for _ in range(2):
        x, branch = t["x"].to(dev).requires_grad_(True), t["branch"].to(dev).requires_grad_(True)
        s, y = layernorm.add_layer_norm_rows(x, branch, scale.to(dev), w, b, EPS, BF16)
        runs.append(torch.autograd.grad([s, y], [x, branch, w, b], [t["dsum"].to(dev), t["dy"].to(dev)]) + (s.detach(), y.detach()))
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    # and the values are right at this size too
    xr, br, sr = _ref_add(t, scale)
    wr, bb = w.detach().double().cpu().requires_grad_(True), b.detach().double().cpu().requires_grad_(True)
    yr = ref_norm(sr, wr, bb)[0]
    want = torch.autograd.grad([sr, yr], [xr, br, wr, bb], [t["dsum"].double(), t["dy"].double()])
    for name, got, ref in zip(("dx", "dbranch", "dgamma", "dbeta"), runs[0], want):
        check(name, got, ref)


# ------------------------------------------------------------------------------------------------ 4. frozen affine
def test_frozen_affine_and_no_grad(dev, monkeypatch):
    C, M = 192, 300
    g = torch.Generator().manual_seed(0)
    x0 = (3.0 + 2.0 * torch.randn(M, C, generator=g)).to(dev)
    dy = torch.randn(M, C, generator=g).to(dev)
    w, b = params(C, dev, 5)
    x = x0.clone().requires_grad_(True)
    w.requires_grad_(True), b.requires_grad_(True)
    layernorm.layer_norm_rows(x, w, b, EPS).backward(dy)
    dx_trained = x.grad.clone()
    assert w.grad is not None and b.grad is not None

    wf, bf = w.detach().clone(), b.detach().clone()
    x = x0.clone().requires_grad_(True)
    parts = []
    real = _lib.call
    spy = lambda name, *a: (parts.append(a[14]) if name == "bfhip_layernorm_bwd" else None, real(name, *a))[1]  # noqa: E731
    with monkeypatch.context() as m:
        m.setattr(_lib, "call", spy)
        layernorm.layer_norm_rows(x, wf, bf, EPS).backward(dy)
    assert parts == [None], "the frozen case must not pass a partial buffer"
    assert torch.equal(x.grad, dx_trained)
    assert wf.grad is None and bf.grad is None

    before = dict(layernorm.LAUNCHES)
    y = layernorm.layer_norm_rows(x0, wf, bf, EPS)
    assert y.grad_fn is None and not y.requires_grad
    s, y = layernorm.add_layer_norm_rows(x0, x0, None, wf, bf, EPS)
    assert s.grad_fn is None and y.grad_fn is None
    assert layernorm.scaled_add_rows(x0, x0).grad_fn is None
    assert layernorm.LAUNCHES["bwd"] == before["bwd"] and layernorm.LAUNCHES["fwd"] == before["fwd"] + 3


# ------------------------------------------------------------------------------------------------ 5. support, fallback
def test_support_and_fallback(dev, monkeypatch):
    lib = _lib.load()
    for C in WIDTHS:
        assert lib.bfhip_layernorm_supported(1000, C, 0, 1) == 1 and layernorm.supported(1000, C, F32, BF16)
    for C in (100, 2048, 0):
        assert lib.bfhip_layernorm_supported(1000, C, 0, 0) == 0
    assert lib.bfhip_layernorm_supported(0, 96, 0, 0) == 0 and lib.bfhip_layernorm_supported(1000, 96, 2, 0) == 0
    assert lib.bfhip_layernorm_parts(1000, 100) == 0
    torch.manual_seed(0)
    for C in (100, 2048):
        x = torch.randn(50, C, device=dev)
        w, b = params(C, dev, 6)
        before = dict(layernorm.LAUNCHES)
        assert torch.equal(layernorm.layer_norm_rows(x, w, b, EPS), F.layer_norm(x, (C,), w, b, EPS))
        assert layernorm.LAUNCHES == before
    # a refused call reports through the library's error string
    x = torch.randn(8, 100, device=dev)
    with pytest.raises(RuntimeError, match="layernorm_fwd: unsupported"):
        _lib.call("bfhip_layernorm_fwd", x.data_ptr(), None, None, 1, x.data_ptr(), x.data_ptr(), 8, 100, EPS, 0, 0, 0, None,
                  x.data_ptr(), x.data_ptr(), _lib.stream_of(x))
    # the switch is read at call time
    x = torch.randn(50, 96, device=dev)
    w, b = params(96, dev, 6)
    monkeypatch.setattr(layernorm, "ENABLED", False)
    before = dict(layernorm.LAUNCHES)
    assert torch.equal(layernorm.layer_norm_rows(x, w, b, EPS), F.layer_norm(x, (96,), w, b, EPS))
    assert layernorm.LAUNCHES == before


def test_other_widths_and_guard_bands(dev):
    """Widths between the Swin ones (masked chunks: 8, 104, 1000) and sentinels around every output: nothing outside is written."""
    G = 1024
    for C, M in ((8, 5), (104, 37), (1000, 19)):
        g = torch.Generator().manual_seed(C)
        x = (3.0 + 2.0 * torch.randn(M, C, generator=g)).to(dev)
        br = torch.randn(M, C, generator=g).to(dev)
        w, b = params(C, dev, 7)
        bufs = {k: torch.full((n + 2 * G,), -7.0e7, device=dev) for k, n in (("s", M * C), ("y", M * C), ("st", 2 * M), ("dx", M * C), ("db", M * C))}
        inner = {k: v[G:-G] for k, v in bufs.items()}
        stream = _lib.stream_of(x)
        _lib.call("bfhip_layernorm_fwd", x.data_ptr(), br.data_ptr(), None, 1, w.data_ptr(), b.data_ptr(), M, C, EPS, 0, 0, 0,
                  inner["s"].data_ptr(), inner["y"].data_ptr(), inner["st"].data_ptr(), stream)
        parts = _lib.load().bfhip_layernorm_parts(M, C)
        partial = torch.full((parts * 2 * C + 2 * G,), -7.0e7, device=dev)
        dwb = torch.full((2 * C + 2 * G,), -7.0e7, device=dev)
        dy = torch.randn(M, C, generator=g).to(dev)
        _lib.call("bfhip_layernorm_bwd", inner["s"].data_ptr(), inner["st"].data_ptr(), w.data_ptr(), dy.data_ptr(), None, None, 1, M, C,
                  0, 0, 0, inner["dx"].data_ptr(), inner["db"].data_ptr(), partial[G:-G].data_ptr(), parts, dwb[G:].data_ptr(),
                  dwb[G + C:].data_ptr(), stream)
        torch.cuda.synchronize()
        for k, v in list(bufs.items()) + [("partial", partial), ("dwb", dwb)]:
            assert bool((v[:G] == -7.0e7).all()) and bool((v[-G:] == -7.0e7).all()), (C, k)
            assert bool((v[G:-G] != -7.0e7).all()), (C, k)
        sr = (x.double() + br.double()).cpu().requires_grad_(True)
        wr = w.double().cpu().requires_grad_(True)
        yr = ref_norm(sr, wr, b.double().cpu())[0]
        dsr, dwr = torch.autograd.grad(yr, [sr, wr], dy.double().cpu())
        check("y", inner["y"].view(M, C), yr)
        check("dx", inner["dx"].view(M, C), dsr)
        assert torch.equal(inner["dx"], inner["db"])
        check("dgamma", dwb[G:G + C], dwr)
        check("dbeta", dwb[G + C:G + 2 * C], dy.double().cpu().sum(0))


# ------------------------------------------------------------------------------------------------ 6. block level
def _run_block(blk, x0, g, seed, on, monkeypatch):
    monkeypatch.setattr(layernorm, "ENABLED", on)
    for p in blk.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    torch.manual_seed(seed)
    before = dict(layernorm.LAUNCHES)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    fwd_launches = layernorm.LAUNCHES["fwd"] - before["fwd"]
    out.backward(g)
    names = ["out", "x"] + [n for n, _ in sorted(blk.named_parameters())]
    vals = [out.detach(), x.grad] + [p.grad.clone() for _, p in sorted(blk.named_parameters())]
    return dict(zip(names, vals)), fwd_launches


def test_swin_block_kernels_on_against_off(dev, monkeypatch):
    torch.manual_seed(0)
    blk = swin.SwinBlock(96, 3, 384, drop_path_rate=0.5).to(dev).train()
    with torch.no_grad():
        for n in (blk.norm1, blk.norm2):
            n.weight.uniform_(0.5, 1.5)
            n.bias.uniform_(-0.5, 0.5)
    x0 = torch.randn(2, 14, 21, 96, device=dev)
    g = torch.randn(2, 14, 21, 96, device=dev)
    for seed in (0, 1, 2):  # different draws of the two drop-path masks; the same samples must drop on both paths
        on, launches = _run_block(blk, x0, g, seed, True, monkeypatch)
        assert launches == 3, launches
        off, launches = _run_block(blk, x0, g, seed, False, monkeypatch)
        assert launches == 0
        assert out_dtype_ok(on["out"], off["out"])
        errs = {k: rel(on[k].float(), off[k].float()) for k in on}
        print("swin block seed", seed, {k: "%.1e" % v for k, v in errs.items()})
        assert all(e < 3e-2 for e in errs.values()), errs
        blk.with_cp = True
        cp, _ = _run_block(blk, x0, g, seed, True, monkeypatch)
        blk.with_cp = False
        for k in on:
            assert torch.equal(cp[k], on[k]), k


def out_dtype_ok(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and a.is_contiguous()


def test_backbone_norms_take_the_kernel(dev, monkeypatch):
    """Patch-embedding, patch-merging and output norms: same dtypes and values with the switch on and off; 2 + 3 * blocks launches."""
    torch.manual_seed(0)
    net = swin.SwinTransformer(embed_dims=96, depths=[1, 1, 1, 1], num_heads=[3, 6, 12, 24], out_indices=[1, 2, 3],
                               drop_path_rate=0.0).to(dev).train()
    x = torch.randn(2, 3, 64, 96, device=dev)
    outs, dense = {}, []
    net.patch_embed.projection.register_forward_hook(lambda m, i, o: dense.append(o.permute(0, 2, 3, 1).is_contiguous()))
    for on in (True, False):
        monkeypatch.setattr(layernorm, "ENABLED", on)
        before = dict(layernorm.LAUNCHES)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs[on] = net(x)
        n = layernorm.LAUNCHES["fwd"] - before["fwd"]
        # 3 mergings, 3 output norms, 3 per block, and the patch embedding's when the convolution returned a channels-last map
        assert n == ((3 + 3 + 4 * 3 + int(dense[-1])) if on else 0), (n, dense)
    for a, b in zip(outs[True], outs[False]):
        assert a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride()
        assert rel(a.float(), b.float()) < 3e-2
