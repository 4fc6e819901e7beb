"""GPU: fused shifted-window attention (csrc/swin_attn.hip) against the fp32 reference of tests/test_swin_cpu.py on the same
bf16 inputs, and the Swin backbone on its HIP path against the same modules on the CPU in fp32.

Tolerances are the project's own for fused attention (tests/test_attn_gpu.py): 2e-2 of the output scale forward, 3e-2 of each
gradient's scale backward -- the probabilities are rounded to bf16 (2^-9 relative) in front of the second matrix product, and
so are the outputs.  Tolerances cannot see a swapped row, so placement is also checked bit for bit with a one-hot softmax."""
import copy
import os
import subprocess
import sys

import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib, swin
from bevfusion_amd.registry import MODELS
from test_swin_cpu import WS, ref_core, ref_regions, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (B, Hp, Wp, heads, shift, extra token pitch); the last case has more windows than the launch has waves (grid loop)
CASES = [(2, 14, 21, 3, 0, 0), (2, 14, 21, 3, 3, 8), (1, 7, 7, 6, 3, 0), (2, 21, 14, 24, 3, 0), (3, 70, 182, 3, 3, 0)]


def make_qkv(B, Hp, Wp, heads, extra, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    C = heads * 32
    buf = torch.randn(B, Hp, Wp, 3 * C + extra, generator=g).to(dev).to(torch.bfloat16)
    return buf[..., :3 * C] if extra else buf


@pytest.mark.parametrize("B,Hp,Wp,heads,shift,extra", CASES)
def test_kernel_matches_reference(dev, B, Hp, Wp, heads, shift, extra):
    C = heads * 32
    qkv = make_qkv(B, Hp, Wp, heads, extra, dev, seed=Hp + heads).requires_grad_(True)
    assert (qkv.stride(2) > 3 * C) == bool(extra)
    g = torch.Generator(device="cpu").manual_seed(1)
    bias = (0.5 * torch.randn(heads, 49, 49, generator=g)).to(dev).requires_grad_(True)
    dout = torch.randn(B, Hp, Wp, C, generator=g).to(dev).to(torch.bfloat16)
    out = swin.window_attention(qkv, bias, heads, shift)
    assert out.dtype == torch.bfloat16 and out.shape == (B, Hp, Wp, C)
    dqkv, dbias = torch.autograd.grad(out, [qkv, bias], dout)
    qr, br = qkv.detach().float().requires_grad_(True), bias.detach().clone().requires_grad_(True)
    ref = ref_core(qr, br, heads, shift)
    dqr, dbr = torch.autograd.grad(ref, [qr, br], dout.float())
    errs = dict(out=rel(out.float(), ref), dq=rel(dqkv[..., :C].float(), dqr[..., :C]), dk=rel(dqkv[..., C:2 * C].float(), dqr[..., C:2 * C]),
                dv=rel(dqkv[..., 2 * C:].float(), dqr[..., 2 * C:]), dqkv=rel(dqkv.float(), dqr), dbias=rel(dbias, dbr))
    print("swin kernel", (B, Hp, Wp, heads, shift, extra), {k: "%.2e" % v for k, v in errs.items()})
    assert errs["out"] < 2e-2
    for k in ("dq", "dk", "dv", "dqkv", "dbias"):
        assert errs[k] < 3e-2, (k, errs)


def one_hot_bias(heads, dy, dx, dev):
    """+60 where the key sits at offset (dy, dx) from the query inside the window, -60 elsewhere."""
    t = torch.arange(49)
    y, x = t // 7, t % 7
    hit = ((y[None, :] - y[:, None]) == dy) & ((x[None, :] - x[:, None]) == dx)  # [query, key]
    return torch.where(hit, 60.0, -60.0)[None].repeat(heads, 1, 1).to(dev)


@pytest.mark.parametrize("shift", [0, 3])
def test_placement_is_bit_exact(dev, shift):
    B, Hp, Wp, heads = 2, 14, 21, 3
    C = heads * 32
    qkv = make_qkv(B, Hp, Wp, heads, 0, dev, seed=5)
    v = qkv[..., 2 * C:]
    # P = identity: every token gets its own v back, exactly
    out = swin.window_attention(qkv, one_hot_bias(heads, 0, 0, dev), heads, shift)
    assert torch.equal(out, v)
    # P = "right-hand neighbour": exact wherever that neighbour shares window and region, per the reference's region map
    bias = one_hot_bias(heads, 0, 1, dev)
    out = swin.window_attention(qkv, bias, heads, shift)
    ref = ref_core(qkv.float(), bias, heads, shift)
    reg = ref_regions(Hp, Wp, shift) if shift else torch.zeros(Hp, Wp, dtype=torch.long)  # indexed by ROLLED coordinates
    uw = (torch.arange(Wp) - shift) % Wp                                                     # rolled column of real column w
    uh = (torch.arange(Hp) - shift) % Hp
    has = (uw % WS != WS - 1)[None, :].expand(Hp, Wp)
    same = reg[uh][:, uw] == reg[uh][:, (uw + 1) % Wp]
    exact = (has & same).to(dev)
    assert 0 < int(exact.sum()) < Hp * Wp
    right = torch.roll(v, shifts=-1, dims=2)
    assert torch.equal(out[:, exact], right[:, exact])
    assert rel(out[:, ~exact].float(), ref[:, ~exact]) < 2e-2


def test_guard_bands_and_full_coverage(dev):
    B, Hp, Wp, heads, shift = 2, 14, 21, 3, 3
    C, G = heads * 32, 4096
    T = B * Hp * Wp
    qkv = make_qkv(B, Hp, Wp, heads, 0, dev, seed=7)
    bias = torch.zeros(heads, 49, 49, device=dev)
    out = torch.full((T * C + 2 * G,), 0x7B7B, dtype=torch.int16, device=dev)
    lse = torch.full((T * heads + 2 * G,), -7.0e7, device=dev)
    dq = torch.full((T * 3 * C + 2 * G,), 0x7B7B, dtype=torch.int16, device=dev)
    dq[G:-G] = 0x7FC0                                                           # bf16 NaN: every element must be written
    stream = _lib.stream_of(qkv)
    _lib.call("bfhip_swin_attn_fwd", qkv.data_ptr(), 3 * C, bias.data_ptr(), B, Hp, Wp, heads, shift, 32 ** -0.5,
              out[G:].data_ptr(), lse[G:].data_ptr(), stream)
    parts = _lib.load().bfhip_swin_attn_parts(B, Hp, Wp, heads)
    partial = torch.full((parts * heads * 2401 + 2 * G,), -7.0e7, device=dev)
    dout = torch.randn(T * C, device=dev).to(torch.bfloat16)
    _lib.call("bfhip_swin_attn_bwd", qkv.data_ptr(), 3 * C, bias.data_ptr(), out[G:].data_ptr(), dout.data_ptr(), lse[G:].data_ptr(),
              B, Hp, Wp, heads, shift, 32 ** -0.5, dq[G:].data_ptr(), partial[G:].data_ptr(), parts, stream)
    torch.cuda.synchronize()
    for name, buf, sentinel in (("out", out, 0x7B7B), ("lse", lse, -7.0e7), ("dqkv", dq, 0x7B7B), ("dbias_partial", partial, -7.0e7)):
        assert bool((buf[:G] == sentinel).all()) and bool((buf[-G:] == sentinel).all()), name
    assert torch.isfinite(dq[G:-G].view(torch.bfloat16).float()).all()
    assert torch.isfinite(out[G:-G].view(torch.bfloat16).float()).all() and torch.isfinite(lse[G:-G]).all()
    assert bool((partial[G:-G] != -7.0e7).all())
    ref = ref_core(qkv.float(), bias, heads, shift)
    assert rel(out[G:-G].view(torch.bfloat16).float().view_as(ref), ref) < 2e-2


def test_backward_is_reproducible(dev):
    B, Hp, Wp, heads, shift = 3, 70, 182, 3, 3
    C = heads * 32
    qkv = make_qkv(B, Hp, Wp, heads, 0, dev, seed=9)
    w = swin.WindowMSA(C, heads, WS).to(dev)
    dout = torch.randn(B, Hp, Wp, C, device=dev).to(torch.bfloat16)
    runs = []
    for _ in range(2):
        q = qkv.detach().clone().requires_grad_(True)
        w.relative_position_bias_table.grad = None
        out = swin.window_attention(q, w.dense_bias(), heads, shift)
        out.backward(dout)
        runs.append((out.detach(), q.grad, out.grad_fn.partial if hasattr(out.grad_fn, "partial") else None,
                     w.relative_position_bias_table.grad.clone()))
    for a, b in zip(*runs):
        assert a is not None and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ module path
def _msa_pair(heads, shift, dev, seed):
    torch.manual_seed(seed)
    m = swin.ShiftWindowMSA(heads * 32, heads, WS, shift_size=shift)
    with torch.no_grad():
        m.w_msa.relative_position_bias_table.normal_(0, 0.5)
        m.w_msa.qkv.bias.normal_(0, 0.3)
        m.w_msa.qkv.weight.normal_(0, 0.15)
        m.w_msa.proj.bias.normal_(0, 0.3)
    return m, copy.deepcopy(m).to(dev)


def _run_msa(m, x, g, autocast):
    x = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        out = m(x)
    params = [p for _, p in sorted(m.named_parameters())]
    grads = torch.autograd.grad(out, [x] + params, g.to(out.dtype))
    return [out.detach().float().cpu()] + [t.float().cpu() for t in grads]


@pytest.mark.parametrize("hw,shift", [((12, 17), 3), ((14, 21), 0), ((14, 21), 3)])
def test_module_hip_path_matches_cpu_fp32(dev, hw, shift, monkeypatch):
    calls = []
    real = swin.window_attention
    monkeypatch.setattr(swin, "window_attention", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    cpu, gpu = _msa_pair(3, shift, dev, seed=hw[0] + shift)
    x = torch.randn(2, hw[0], hw[1], 96)
    g = torch.randn(2, hw[0], hw[1], 96)
    want = _run_msa(cpu, x, g, False)
    got = _run_msa(gpu, x.to(dev), g.to(dev), True)
    assert calls, "the HIP path was not taken"
    names = ["out", "x"] + [n for n, _ in sorted(cpu.named_parameters())]
    errs = {n: rel(a, b) for n, a, b in zip(names, got, want)}
    print("swin module", hw, shift, {k: "%.2e" % v for k, v in errs.items()})
    assert all(e < 3e-2 for e in errs.values()), errs


def test_torch_path_in_a_child_process_agrees(dev, tmp_path):
    """BFHIP_SWIN_ATTN=0 (read at import) routes the same module through its plain-torch path."""
    cpu, gpu = _msa_pair(3, 3, dev, seed=11)
    x, g = torch.randn(2, 12, 17, 96), torch.randn(2, 12, 17, 96)
    torch.save(dict(state=cpu.state_dict(), x=x, g=g), tmp_path / "in.pt")
    code = r"""
import sys, torch
sys.path.insert(0, %r)
import bevfusion_amd
from bevfusion_amd import swin
assert not swin.ENABLED
d = torch.load(%r)
m = swin.ShiftWindowMSA(96, 3, 7, shift_size=3)
m.load_state_dict(d["state"])
m = m.cuda()
assert not m.hip_eligible(d["x"].cuda())
x = d["x"].cuda().requires_grad_(True)
with torch.autocast("cuda", dtype=torch.bfloat16):
    out = m(x)
params = [p for _, p in sorted(m.named_parameters())]
grads = torch.autograd.grad(out, [x] + params, d["g"].cuda().to(out.dtype))
torch.save([out.detach().float().cpu()] + [t.float().cpu() for t in grads], %r)
print("TORCH_PATH_OK")
""" % (ROOT, str(tmp_path / "in.pt"), str(tmp_path / "out.pt"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, BFHIP_SWIN_ATTN="0"))
    assert r.returncode == 0 and "TORCH_PATH_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    want = torch.load(tmp_path / "out.pt")
    got = _run_msa(gpu, x.to(dev), g.to(dev), True)
    for i, (a, b) in enumerate(zip(got, want)):
        assert rel(a, b) < 3e-2, i


# ------------------------------------------------------------------------------------------------ whole backbone
def test_backbone_matches_cpu_fp32(dev, monkeypatch):
    calls = []
    real = swin.window_attention
    monkeypatch.setattr(swin, "window_attention", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(0)
    cpu = swin.SwinTransformer(embed_dims=96, depths=[2, 2, 2, 2], num_heads=[3, 6, 12, 24], out_indices=[1, 2, 3],
                               drop_path_rate=0.0).train()
    gpu = copy.deepcopy(cpu).to(dev).train()
    x = torch.randn(2, 3, 64, 96)
    outs_c = cpu(x)
    ws = [torch.randn_like(o) for o in outs_c]
    sum((o * w).sum() for o, w in zip(outs_c, ws)).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        outs_g = gpu(x.to(dev))
    assert len(calls) == 8
    sum((o.float() * w.to(dev)).sum() for o, w in zip(outs_g, ws)).backward()
    l2 = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    for i, (a, b) in enumerate(zip(outs_g, outs_c)):
        assert a.shape == b.shape and a.permute(0, 2, 3, 1).is_contiguous()
        e = l2(a.detach().float().cpu(), b.detach())
        print("swin backbone out", i, "%.2e" % e)
        assert e < 3e-2, (i, e)
    worst = (1.0, None)
    for (n, p), q in zip(cpu.named_parameters(), gpu.parameters()):
        assert q.grad is not None and torch.isfinite(q.grad).all(), n
        cos = float(torch.nn.functional.cosine_similarity(q.grad.float().cpu().reshape(-1), p.grad.reshape(-1), dim=0))
        worst = min(worst, (cos, n))
        assert cos >= 0.99, (n, cos)
    print("swin backbone worst gradient cosine", worst)
    # eval + no_grad still runs the kernels
    del calls[:]
    cpu.eval(), gpu.eval()
    with torch.no_grad():
        want = cpu(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got = gpu(x.to(dev))
    assert len(calls) == 8
    for a, b in zip(got, want):
        assert l2(a.float().cpu(), b) < 3e-2


def test_full_model_with_swin_trains_one_step(dev):
    from bevfusion_amd import synthetic
    from bevfusion_amd.amp import MasterWeightAdamW
    from bevfusion_amd.bevfusion import nuscenes_config
    from test_model_gpu import _inputs
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config(img_backbone="swin_t")).to(dev).train()
    model.view_transform.conv_dtype = torch.bfloat16
    opt = MasterWeightAdamW(model, lr=2e-4, weight_decay=0.01, max_grad_norm=35.0)
    bb = model.img_backbone
    assert bb.stages[0].blocks[0].attn.w_msa.qkv.weight.dtype == torch.bfloat16
    assert bb.stages[0].blocks[0].attn.w_msa.relative_position_bias_table.dtype == torch.float32
    assert bb.stages[0].blocks[0].norm1.weight.dtype == torch.float32
    before = {n: p.detach().clone() for n, p in bb.named_parameters()}
    inp = _inputs(dev, 1)
    gts = [tuple(torch.from_numpy(a) for a in synthetic.gt_boxes(seed=3000))]
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        losses = model.loss(inp, gts)
        total, _ = model.parse_losses(losses)
    assert torch.isfinite(total)
    total.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in bb.parameters())
    opt.step()
    torch.cuda.synchronize()
    assert float(opt.scalars[1]) == 0.0 if opt.flat else True
    same = [n for n, p in bb.named_parameters() if torch.equal(p.detach(), before[n])]
    assert not same, same
