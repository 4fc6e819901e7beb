"""Shifted-window attention (csrc/swin_attn.hip) against the module's own plain-torch path, and one whole backbone
forward + backward, at the four stage shapes of a batch of 24 images of 256 x 704 (token maps 64 x 176, 32 x 88, 16 x 44, 8 x 22
with 3, 6, 12, 24 heads; padded to multiples of 7 as the module pads them).

HIP events around every iteration, warm-up, median of many iterations; both paths in one process, interleaved by shape.
Writes profiles/swin_micro.json.  Usage: python tools/swin_micro.py [--iters 30] [--out profiles/swin_micro.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bevfusion_amd  # noqa: E402,F401
from bevfusion_amd import swin  # noqa: E402
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


def backbone_rows(iters, dev):
    x = torch.randn(BATCH, 3, 256, 704, device=dev)
    out = {}

    def step(model):
        def run():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                outs = model(x)
                loss = sum(o.float().square().mean() for o in outs)
            loss.backward()
            for p in model.parameters():
                p.grad = None
        return run

    torch.manual_seed(0)
    sw = swin.SwinTransformer(embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], out_indices=[1, 2, 3],
                              drop_path_rate=0.2).to(dev).train()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "swin_micro.json"))
    ap.add_argument("--skip-backbone", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), batch=BATCH, image=[256, 704], iters=args.iters, hbm_peak_bytes_per_s=HBM_PEAK,
               attention=attention_rows(args.iters, dev))
    if not args.skip_backbone:
        res["backbone"] = backbone_rows(max(args.iters // 3, 5), dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
