#!/usr/bin/env python3
"""GPU time of the decoder's cross attention (8 heads x 16, batch 4, 32 400 keys), forward and forward + backward.

Default: 200 queries (the nuScenes head), dropout 0.1 and 0, by graph replay.
--wide [OUT.json]: 500 queries (the custom_data head), dropout 0.1: the split-key kernels against the library's
scaled_dot_product_attention on the same tensors in the same process, timed eagerly between HIP events (both sides take
milliseconds, far above the host's dispatch time); the result is printed and, with a path, written as JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import attention
from resnet_conv_micro import timed

dev = torch.device("cuda:0")
H, D = 8, 16


def tensors(B, Lq, Lk):
    q = torch.randn(B, Lq, H * D, device=dev).to(torch.bfloat16).requires_grad_(True)
    k = torch.randn(B, Lk, H * D, device=dev).to(torch.bfloat16).requires_grad_(True)
    v = torch.randn(B, Lk, H * D, device=dev).to(torch.bfloat16).requires_grad_(True)
    g = torch.randn(B, Lq, H * D, device=dev).to(torch.bfloat16)
    return q, k, v, g


def event_timed(fn, warmup=3, iters=10, reps=5):
    """ms per call: best of `reps` runs of `iters` eager calls between two HIP events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def sdpa(q, k, v, p):
    """What _MHA.attend runs when the kernels do not take the shape."""
    B, Lq, E = q.shape
    heads = lambda t: t.view(B, -1, H, E // H).transpose(1, 2)  # noqa: E731
    o = torch.nn.functional.scaled_dot_product_attention(heads(q), heads(k), heads(v), dropout_p=p)
    return o.transpose(1, 2).reshape(B, Lq, E)


def wide(out_path):
    B, Lq, Lk, p = 4, 500, 32400, 0.1
    q, k, v, g = tensors(B, Lq, Lk)
    assert attention.supported_wide(q, k, v, H)
    res = dict(shape=dict(B=B, H=H, Lq=Lq, Lk=Lk, head_dim=D), dropout=p, method="eager, HIP events, best of 5 x 10 calls",
               device=torch.cuda.get_device_name(0))
    for name, fn in (("kernel", lambda a, b, c: attention.cross_attention(a, b, c, H, dropout_p=p, seed=7)),
                     ("sdpa", lambda a, b, c: sdpa(a, b, c, p))):
        fwd = event_timed(lambda: fn(q.detach(), k.detach(), v.detach()))
        fb = event_timed(lambda: torch.autograd.grad(fn(q, k, v), (q, k, v), g))
        res[name] = dict(fwd_ms=round(fwd, 4), fwd_bwd_ms=round(fb, 4), bwd_ms=round(fb - fwd, 4))
        print("%-6s fwd %.4f ms   fwd+bwd %.4f ms   bwd %.4f ms" % (name, fwd, fb, fb - fwd))
    res["speedup"] = dict(fwd=round(res["sdpa"]["fwd_ms"] / res["kernel"]["fwd_ms"], 3),
                          bwd=round(res["sdpa"]["bwd_ms"] / res["kernel"]["bwd_ms"], 3))
    res["workspace_bytes"] = attention._lib.call_size("bfhip_attn_workspace_bytes", B, H, Lq, Lk)
    print(json.dumps(res))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if "--wide" in sys.argv:
    i = sys.argv.index("--wide")
    wide(sys.argv[i + 1] if len(sys.argv) > i + 1 else None)
else:
    q, k, v, g = tensors(4, 200, 32400)
    for p in (0.1, 0.0):
        fwd = timed(lambda: attention.cross_attention(q.detach(), k.detach(), v.detach(), H, dropout_p=p, seed=7))
        fb = timed(lambda: torch.autograd.grad(attention.cross_attention(q, k, v, H, dropout_p=p, seed=7), (q, k, v), g))
        print("dropout %.1f: fwd %.4f ms   fwd+bwd %.4f ms   bwd %.4f ms" % (p, fwd, fb, fb - fwd))
