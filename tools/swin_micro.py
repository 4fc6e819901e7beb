"""Shifted-window attention (csrc/swin_attn.hip) against the module's own plain-torch path, and one whole backbone
forward + backward, at the four stage shapes of a batch of 24 images of 256 x 704 (token maps 64 x 176, 32 x 88, 16 x 44, 8 x 22
with 3, 6, 12, 24 heads; padded to multiples of 7 as the module pads them).

HIP events around every iteration, warm-up, median of many iterations; both paths in one process, interleaved by shape.
Writes profiles/swin_micro.json.  Usage: python tools/swin_micro.py [--iters 30] [--out profiles/swin_micro.json]

--ln: the LayerNorm / residual kernels (csrc/layernorm.hip) instead: norm, add + norm and add at the four stage token matrices
(C = 96 / 192 / 384 / 768; fp32 stream, bf16 branch and norm output as in the block under autocast), kernel against the torch
sequence it replaces (the same functions with layernorm.ENABLED off), forward and backward; then the whole backbone with the
switch off and on, interleaved (--pairs runs each), and with --custom-step one tools/custom_step.py run each way at batch 1
(child processes, BFHIP_SWIN_LN=0 / 1).  Writes profiles/swin_ln_micro.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bevfusion_amd  # noqa: E402,F401
from bevfusion_amd import layernorm, swin  # noqa: E402
from bevfusion_amd.dense_modules import ResNet50  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X datasheet
STAGES = [(64, 176, 3), (32, 88, 6), (16, 44, 12), (8, 22, 24)]
BATCH = 24


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def torch_core(msa, qkv, bias):
    """What ShiftWindowMSA._forward_torch does between the qkv Linear and the projection, on an already padded qkv map."""
    B, Hp, Wp, C3 = qkv.shape
    C, ws, s, heads = C3 // 3, msa.window_size, msa.shift_size, msa.w_msa.num_heads
    mask = None
    if s > 0:
        qkv = torch.roll(qkv, shifts=(-s, -s), dims=(1, 2))
        img = torch.zeros((1, Hp, Wp, 1), device=qkv.device)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
            for wsl in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                img[:, hs, wsl, :] = cnt
                cnt += 1
        mw = msa._partition(img).reshape(-1, ws * ws)
        mask = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = mask.masked_fill(mask != 0, -100.0)
    w = msa._partition(qkv).reshape(-1, ws * ws, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = w[0] * msa.w_msa.scale, w[1], w[2]
    attn = q @ k.transpose(-2, -1) + bias.to(q.dtype).unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = (attn.view(-1, nW, heads, ws * ws, ws * ws) + mask.to(attn.dtype).unsqueeze(1).unsqueeze(0)).view(-1, heads, ws * ws, ws * ws)
    out = (torch.softmax(attn, -1) @ v).transpose(1, 2).reshape(-1, ws, ws, C)
    out = out.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    return torch.roll(out, shifts=(s, s), dims=(1, 2)) if s > 0 else out


def attention_rows(iters, dev):
    rows = []
    for H, W, heads in STAGES:
        Hp, Wp, C = -(-H // 7) * 7, -(-W // 7) * 7, heads * 32
        for shift in (0, 3):
            msa = swin.ShiftWindowMSA(C, heads, 7, shift_size=shift).to(dev)
            qkv = torch.randn(BATCH, Hp, Wp, 3 * C, device=dev).to(torch.bfloat16).requires_grad_(True)
            bias = msa.w_msa.dense_bias().detach().requires_grad_(True)
            dout = torch.randn(BATCH, Hp, Wp, C, device=dev).to(torch.bfloat16)
            tok = BATCH * Hp * Wp
            fwd_bytes = tok * (3 * C * 2 + C * 2 + heads * 4)
            bwd_bytes = fwd_bytes + tok * (C * 2 + 3 * C * 2)
            row = dict(tokens=[H, W], padded=[Hp, Wp], heads=heads, shift=shift, fwd_bytes=fwd_bytes, bwd_bytes=bwd_bytes)
            for name, f in (("hip", lambda: swin.window_attention(qkv, bias, heads, shift)), ("torch", lambda: torch_core(msa, qkv, bias))):
                out = f()
                row[name + "_fwd_ms"], row[name + "_fwd_min_ms"] = timed(f, iters)
                g = lambda: torch.autograd.grad(out, [qkv, bias], dout, retain_graph=True)  # noqa: E731
                row[name + "_bwd_ms"], row[name + "_bwd_min_ms"] = timed(g, iters)
                del out
            row["hip_fwd_hbm_fraction"] = fwd_bytes / (row["hip_fwd_ms"] * 1e-3) / HBM_PEAK
            row["hip_bwd_hbm_fraction"] = bwd_bytes / (row["hip_bwd_ms"] * 1e-3) / HBM_PEAK
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def backbone_step(model, x):
    def run():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs = model(x)
            loss = sum(o.float().square().mean() for o in outs)
        loss.backward()
        for p in model.parameters():
            p.grad = None
    return run


def swin_t(dev):
    torch.manual_seed(0)
    return swin.SwinTransformer(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], out_indices=[1, 2, 3],
                                drop_path_rate=0.2).to(dev).train()


def backbone_rows(iters, dev):
    x = torch.randn(BATCH, 3, 256, 704, device=dev)
    out = {}
    step = lambda model: backbone_step(model, x)  # noqa: E731
    sw = swin_t(dev)
    for name, on in (("swin_t_hip", True), ("swin_t_torch", False)):
        swin.ENABLED = on
        out[name + "_fwd_bwd_ms"], out[name + "_fwd_bwd_min_ms"] = timed(step(sw), iters, warmup=3)
        print(name, out[name + "_fwd_bwd_ms"], flush=True)
    swin.ENABLED = True
    del sw
    rn = ResNet50().to(dev).train()
    out["resnet50_fwd_bwd_ms"], out["resnet50_fwd_bwd_min_ms"] = timed(step(rn), iters, warmup=3)
    print("resnet50", out["resnet50_fwd_bwd_ms"], flush=True)
    return out


# ------------------------------------------------------------------------------------------------ --ln
def ln_op_rows(iters, dev):
    """Per stage and op: kernel (layernorm.ENABLED on) and torch sequence (off) through the same three functions.  Algorithmic
    bytes per element of the [M, C] matrix: f32 stream 4, bf16 branch / norm output 2 (statistics and parameters left out)."""
    F32, BF16 = torch.float32, torch.bfloat16
    rows = []
    for H, W, heads in STAGES:
        C, M = heads * 32, BATCH * H * W
        x = (3.0 + 2.0 * torch.randn(BATCH, H, W, C, device=dev)).requires_grad_(True)
        br = torch.randn(BATCH, H, W, C, device=dev).to(BF16).requires_grad_(True)
        w = (1.0 + 0.1 * torch.randn(C, device=dev)).requires_grad_(True)
        b = (0.1 * torch.randn(C, device=dev)).requires_grad_(True)
        scale = (torch.rand(BATCH, device=dev) < 0.8).float() / 0.8
        dsum, dy = torch.randn(BATCH, H, W, C, device=dev), torch.randn(BATCH, H, W, C, device=dev).to(BF16)
        ops = dict(
            norm=(lambda: (layernorm.layer_norm_rows(x, w, b, 1e-5, BF16),), [x, w, b], [dy], 4 + 2, 4 + 2 + 4),
            add_norm=(lambda: layernorm.add_layer_norm_rows(x, br, scale, w, b, 1e-5, BF16), [x, br, w, b], [dsum, dy],
                      4 + 2 + 4 + 2, 4 + 2 + 4 + 4 + 2),
            add=(lambda: (layernorm.scaled_add_rows(x, br, scale),), [x, br], [dsum], 4 + 2 + 4, 4 + 2))
        for op, (f, inputs, grads, fb, bb) in ops.items():
            row = dict(op=op, tokens=[H, W], M=M, C=C, fwd_bytes=M * C * fb, bwd_bytes=M * C * bb)
            for name, on in (("hip", True), ("torch", False)):
                layernorm.ENABLED = on
                outs = f()
                row[name + "_fwd_ms"], row[name + "_fwd_min_ms"] = timed(f, iters)
                g = lambda: torch.autograd.grad(outs, inputs, grads, retain_graph=True)  # noqa: E731
                row[name + "_bwd_ms"], row[name + "_bwd_min_ms"] = timed(g, iters)
                del outs
            layernorm.ENABLED = True
            row["hip_fwd_hbm_fraction"] = row["fwd_bytes"] / (row["hip_fwd_ms"] * 1e-3) / HBM_PEAK
            row["hip_bwd_hbm_fraction"] = row["bwd_bytes"] / (row["hip_bwd_ms"] * 1e-3) / HBM_PEAK
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def ln_backbone_pairs(iters, pairs, dev):
    """Swin-T forward + backward (bf16 autocast, drop path 0.2) with the switch off and on, interleaved: off, on, off, on, .."""
    x = torch.randn(BATCH, 3, 256, 704, device=dev)
    run = backbone_step(swin_t(dev), x)
    out = dict(off_ms=[], on_ms=[], iters=iters)
    for _ in range(pairs):
        for name, on in (("off_ms", False), ("on_ms", True)):
            layernorm.ENABLED = on
            out[name].append(timed(run, iters, warmup=3)[0])
            print("swin_t fwd+bwd, BFHIP_SWIN_LN", int(on), out[name][-1], flush=True)
    layernorm.ENABLED = True
    out["every_on_run_below_every_off_run"] = max(out["on_ms"]) < min(out["off_ms"])
    return out


def ln_custom_step_pair():
    out = {}
    for name, flag in (("off", "0"), ("on", "1")):
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "step.json")
            subprocess.run([sys.executable, os.path.join(ROOT, "tools", "custom_step.py"), path, "--batches", "1"], check=True,
                           env=dict(os.environ, BFHIP_SWIN_LN=flag), timeout=600)
            with open(path) as f:
                out[name] = json.load(f)["runs"][0]
    return out


def ln_main(args):
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), batch=BATCH, image=[256, 704], iters=args.iters, hbm_peak_bytes_per_s=HBM_PEAK,
               ops=ln_op_rows(args.iters, dev))
    if not args.skip_backbone:
        res["backbone"] = ln_backbone_pairs(max(args.iters // 3, 5), args.pairs, dev)
    if args.custom_step:
        res["custom_step_batch1"] = ln_custom_step_pair()
    out = args.out or os.path.join(ROOT, "profiles", "swin_ln_micro.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ln", action="store_true", help="the LayerNorm / residual kernels instead of attention")
    ap.add_argument("--pairs", type=int, default=3, help="--ln: backbone runs each way")
    ap.add_argument("--custom-step", action="store_true", help="--ln: also one tools/custom_step.py run each way")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-backbone", action="store_true")
    args = ap.parse_args()
    if args.ln:
        return ln_main(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "swin_micro.json")
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), batch=BATCH, image=[256, 704], iters=args.iters, hbm_peak_bytes_per_s=HBM_PEAK,
               attention=attention_rows(args.iters, dev))
    if not args.skip_backbone:
        res["backbone"] = backbone_rows(max(args.iters // 3, 5), dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
