"""GPU: split-key cross attention (csrc/attn.hip) with more than 256 queries -- a query-block grid axis in the forward, 32
query tiles per key tile in the backward -- against the fp32 reference and the tolerances of tests/test_attn_gpu.py (2e-2
of the output scale, 3e-2 of the gradient scale: bf16 probabilities feed the second MFMA, whatever the query count)."""
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib
from bevfusion_amd import attention as at
from test_attn_gpu import reference, rel

pytestmark = pytest.mark.gpu


def _qkv(dev, B, H, Lq, Lk, grad=True):
    E = H * 16
    q = (torch.randn(B, Lq, E, device=dev) * 1.5).to(torch.bfloat16).requires_grad_(grad)
    k = (torch.randn(B, Lk, E, device=dev) * 1.5).to(torch.bfloat16).requires_grad_(grad)
    v = torch.randn(B, Lk, E, device=dev).to(torch.bfloat16).requires_grad_(grad)
    return q, k, v


def _check_parity(dev, B, H, Lq, Lk, p):
    torch.manual_seed(0)
    q, k, v = _qkv(dev, B, H, Lq, Lk)
    seed = 1234567
    out = at.cross_attention(q, k, v, H, p, seed)
    mask = at.dropout_mask(B, H, Lq, Lk, p, seed, dev) if p > 0 else None
    if mask is not None:
        rate = float(mask.float().mean())
        print("keep rate", rate)
        assert abs(rate - (1 - p)) < 5e-3
    qr, kr, vr = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    ref = reference(qr, kr, vr, H, mask, p)
    g = torch.randn_like(ref)
    out.backward(g.to(torch.bfloat16))
    ref.backward(g.to(torch.bfloat16).float())
    errs = (rel(out.float(), ref), rel(q.grad.float(), qr.grad), rel(k.grad.float(), kr.grad), rel(v.grad.float(), vr.grad))
    print("rel err out / dQ / dK / dV:", errs)
    assert out.dtype == torch.bfloat16 and errs[0] < 2e-2
    assert errs[1] < 3e-2 and errs[2] < 3e-2 and errs[3] < 3e-2


# Lk = 700: two key chunks, the second ragged; 257: one full query block plus one query; 512: the limit
@pytest.mark.parametrize("B,H,Lq,Lk", [(2, 3, 257, 700), (2, 3, 300, 700), (1, 2, 500, 1100), (2, 8, 512, 2049)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_wide_cross_attention_matches_reference(dev, B, H, Lq, Lk, p):
    _check_parity(dev, B, H, Lq, Lk, p)


def test_wide_cross_attention_at_the_custom_head_shape(dev):
    """500 proposals against the 180 x 180 BEV cells, 8 heads, dropout 0.1 (the reference's custom_data head)."""
    _check_parity(dev, 2, 8, 500, 32400, 0.1)


def test_wide_cross_attention_is_reproducible_and_seeded(dev):
    """Same seed: bit-identical output AND gradients (dK / dV are sums over all 500 queries in a fixed order)."""
    torch.manual_seed(1)
    q, k, v = _qkv(dev, 2, 8, 500, 3000)
    g = torch.randn(2, 500, 128, device=dev).to(torch.bfloat16)
    runs = []
    for seed in (42, 42, 43):
        out = at.cross_attention(q, k, v, 8, 0.1, seed)
        runs.append((out.detach(),) + torch.autograd.grad(out, (q, k, v), g))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], runs[2][0]) and not torch.equal(runs[0][2], runs[2][2])


def test_wide_predicate_and_entry_point_agree_on_the_limit(dev):
    limit = at.max_queries()
    assert limit >= 512
    k = torch.zeros(1, at.MIN_KEYS, 128, device=dev, dtype=torch.bfloat16)

    def q(n):
        return torch.zeros(1, n, 128, device=dev, dtype=torch.bfloat16)

    assert at.supported_wide(q(257), k, k, 8) and at.supported_wide(q(500), k, k, 8)
    assert at.supported_wide(q(limit), k, k, 8) and not at.supported_wide(q(limit + 1), k, k, 8)
    assert not at.supported_wide(q(256), k, k, 8) and at.supported(q(256), k, k, 8)
    assert not at.supported(q(300), k, k, 8)
    assert not at.supported_wide(q(500), k[:, :at.MIN_KEYS - 1], k[:, :at.MIN_KEYS - 1], 8)
    assert not at.supported_wide(q(500).float(), k, k, 8)
    # the C entry point: rc 0 at the limit, refused (before any launch) one above it
    lib = _lib.load()
    for n, ok in ((limit, True), (limit + 1, False)):
        qq, o = q(n), q(n)
        lse = torch.empty(8, n, dtype=torch.float32, device=dev)
        nbytes = _lib.call_size("bfhip_attn_workspace_bytes", 1, 8, n, at.MIN_KEYS)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        rc = lib.bfhip_attn_fwd(qq.data_ptr(), k.data_ptr(), k.data_ptr(), 1, 8, n, at.MIN_KEYS, 0.25, 0.0, 0, None,
                                o.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_of(qq))
        assert (rc == 0) == ok, (n, rc)
        dq, dk, dv = q(n), torch.empty_like(k), torch.empty_like(k)
        rc = lib.bfhip_attn_bwd(qq.data_ptr(), k.data_ptr(), k.data_ptr(), o.data_ptr(), o.data_ptr(), lse.data_ptr(), 1, 8, n,
                                at.MIN_KEYS, 0.25, 0.0, 0, None, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(),
                                ws.numel(), _lib.stream_of(qq))
        assert (rc == 0) == ok, (n, rc)
    torch.cuda.synchronize()
    # the switch for A/B runs turns the wide path off alone
    at.WIDE = False
    try:
        assert not at.supported_wide(q(500), k, k, 8) and at.supported(q(200), k, k, 8)
    finally:
        at.WIDE = True


def test_decoder_layer_takes_the_kernel_at_500_queries(dev, monkeypatch):
    """_MHA, 500 queries against 2304 keys under bf16 autocast: the kernel path equals the library path (ENABLED = False)
    within 2e-2 of the scale, output and the gradient of the packed projection weight alike."""
    from bevfusion_amd.dense_modules import _MHA
    torch.manual_seed(2)
    m = _MHA(128, 8, dropout=0.0).to(dev).train()
    q = torch.randn(2, 500, 128, device=dev)
    k = torch.randn(2, 2304, 128, device=dev)
    g = torch.randn(2, 500, 128, device=dev)
    calls = []
    real = at.cross_attention
    monkeypatch.setattr(at, "cross_attention", lambda *a, **kw: (calls.append(a[0].shape[1]), real(*a, **kw))[1])
    res = []
    for enabled in (True, False):
        monkeypatch.setattr(at, "ENABLED", enabled)
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = m(q, k, k)
        (out.float() * g).sum().backward()
        res.append((out.detach().float(), m.attn.in_proj_weight.grad.detach().float().clone()))
    assert calls == [500]
    e_out, e_w = rel(res[0][0], res[1][0]), rel(res[0][1], res[1][1])
    print("rel err out / d in_proj_weight:", e_out, e_w)
    assert e_out < 2e-2 and e_w < 2e-2
