"""CPU: the Swin-T image backbone (bevfusion_amd/swin.py) on its plain-torch path against an independent reference of
shifted-window attention written here from the published algorithm (pad, roll, partition, an explicitly built mask, softmax,
reverse, roll back, crop), plus the constructor / state-dict / patch-merging / drop-path / config contracts.  The reference
functions are also what tests/test_swin_gpu.py holds the HIP kernels against."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import bevfusion_amd  # noqa: F401
from bevfusion_amd import swin
from bevfusion_amd.registry import MODELS

WS = 7


# ------------------------------------------------------------------------------------------------ independent reference
def ref_partition(x):
    """[B, Hp, Wp, C] -> [B * windows, 49, C], windows row-major."""
    B, Hp, Wp, C = x.shape
    x = x.reshape(B, Hp // WS, WS, Wp // WS, WS, C)
    return x.transpose(2, 3).reshape(-1, WS * WS, C)


def ref_reverse(w, B, Hp, Wp):
    C = w.shape[-1]
    w = w.reshape(B, Hp // WS, Wp // WS, WS, WS, C)
    return w.transpose(2, 3).reshape(B, Hp, Wp, C)


def ref_regions(Hp, Wp, shift):
    """Region id of every position of the ROLLED map: three bands per axis, [0, L-7), [L-7, L-shift), [L-shift, L)."""
    band = lambda L: torch.tensor([0 if u < L - WS else (1 if u < L - shift else 2) for u in range(L)])  # noqa: E731
    return band(Hp)[:, None] * 3 + band(Wp)[None, :]


def ref_mask(Hp, Wp, shift, device):
    """[windows, 49, 49]: -100 where query and key of a window come from different regions, else 0."""
    reg = ref_partition(ref_regions(Hp, Wp, shift).reshape(1, Hp, Wp, 1).float()).squeeze(-1)  # [windows, 49]
    mask = torch.zeros(reg.shape[0], WS * WS, WS * WS)
    mask[reg[:, :, None] != reg[:, None, :]] = -100.0
    return mask.to(device)


def ref_core(qkv, bias, heads, shift):
    """qkv [B, Hp, Wp, 3C] (channel = which * C + head * 32 + d), bias [heads, 49, 49] -> [B, Hp, Wp, C]: the attention
    between the qkv Linear and the projection, window by window."""
    B, Hp, Wp, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    if shift > 0:
        qkv = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2))
    w = ref_partition(qkv)                                            # [Bw, 49, 3C]
    Bw = w.shape[0]
    w = w.reshape(Bw, WS * WS, 3, heads, hd).permute(2, 0, 3, 1, 4)    # [3, Bw, heads, 49, hd]
    q, k, v = w[0] * hd ** -0.5, w[1], w[2]
    attn = q @ k.transpose(-2, -1) + bias[None]
    if shift > 0:
        nW = (Hp // WS) * (Wp // WS)
        m = ref_mask(Hp, Wp, shift, qkv.device).to(attn.dtype)
        attn = (attn.reshape(B, nW, heads, WS * WS, WS * WS) + m[None, :, None]).reshape(Bw, heads, WS * WS, WS * WS)
    attn = torch.softmax(attn, dim=-1)
    out = (attn @ v).transpose(1, 2).reshape(Bw, WS * WS, C)
    out = ref_reverse(out, B, Hp, Wp)
    if shift > 0:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out


def ref_attention(x, qkv_w, qkv_b, proj_w, proj_b, table, index, heads, shift):
    """ShiftWindowMSA on x [B, H, W, C]: pad, roll, partition, window attention with bias and mask, reverse, roll back, crop."""
    B, H, W, C = x.shape
    hd = C // heads
    x = F.pad(x, (0, 0, 0, (WS - W % WS) % WS, 0, (WS - H % WS) % WS))
    Hp, Wp = x.shape[1:3]
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    w = ref_partition(x)
    Bw = w.shape[0]
    qkv = F.linear(w, qkv_w, qkv_b).reshape(Bw, WS * WS, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * hd ** -0.5, qkv[1], qkv[2]
    bias = table[index.reshape(-1)].reshape(WS * WS, WS * WS, heads).permute(2, 0, 1)
    attn = q @ k.transpose(-2, -1) + bias[None]
    if shift > 0:
        nW = (Hp // WS) * (Wp // WS)
        m = ref_mask(Hp, Wp, shift, x.device).to(attn.dtype)
        attn = (attn.reshape(B, nW, heads, WS * WS, WS * WS) + m[None, :, None]).reshape(Bw, heads, WS * WS, WS * WS)
    attn = torch.softmax(attn, dim=-1)
    out = F.linear((attn @ v).transpose(1, 2).reshape(Bw, WS * WS, C), proj_w, proj_b)
    out = ref_reverse(out, B, Hp, Wp)
    if shift > 0:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out[:, :H, :W]


def rel(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ attention parity
@pytest.mark.parametrize("hw,shift,heads", list(itertools.product([(12, 17), (14, 21), (7, 7), (5, 9)], [0, 3], [3, 6])))
def test_torch_path_matches_the_reference(hw, shift, heads):
    torch.manual_seed(hw[0] * 100 + hw[1] + shift + heads)
    C = heads * 32
    m = swin.ShiftWindowMSA(C, heads, WS, shift_size=shift)
    w = m.w_msa
    with torch.no_grad():
        w.relative_position_bias_table.normal_(0, 0.5)
        w.qkv.bias.normal_(0, 0.3)
        w.proj.bias.normal_(0, 0.3)
        w.qkv.weight.normal_(0, 0.15)
    x = torch.randn(2, hw[0], hw[1], C, requires_grad=True)
    params = [w.qkv.weight, w.qkv.bias, w.proj.weight, w.proj.bias, w.relative_position_bias_table]
    out = m(x)
    assert out.shape == x.shape
    g = torch.randn_like(out)
    got = torch.autograd.grad(out, [x] + params, g)
    xr = x.detach().clone().requires_grad_(True)
    pr = [p.detach().clone().requires_grad_(True) for p in params]
    ref = ref_attention(xr, *pr, w.relative_position_index, heads, shift)
    want = torch.autograd.grad(ref, [xr] + pr, g)
    assert rel(out, ref) < 1e-5
    for name, a, b in zip(("x", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias", "table"), got, want):
        assert rel(a, b) < 1e-5, name


def test_fresh_index_buffer_and_loaded_buffer_wins():
    w = swin.WindowMSA(96, 3, WS)
    idx = w.relative_position_index
    assert idx.shape == (49, 49) and idx.dtype == torch.long
    for i, j in ((0, 0), (0, 48), (10, 3), (48, 0)):
        yi, xi, yj, xj = i // 7, i % 7, j // 7, j % 7
        assert int(idx[i, j]) == (yi - yj + 6) * 13 + (xi - xj + 6)
    sd = w.state_dict()
    assert "relative_position_index" in sd
    flipped = idx.flip(0).contiguous()  # some other valid index; the buffer itself is overwritten in place by the load
    sd["relative_position_index"] = flipped
    w.load_state_dict(sd)
    assert torch.equal(w.relative_position_index, flipped)
    with torch.no_grad():
        w.relative_position_bias_table.normal_()
    want = w.relative_position_bias_table[flipped.reshape(-1)].reshape(49, 49, 3).permute(2, 0, 1)
    assert torch.equal(w.dense_bias(), want)
    # the table's gradient through the fixed gather plan equals the index-add of autograd
    t = w.relative_position_bias_table.detach().clone().requires_grad_(True)
    g = torch.randn(3, 49, 49)
    (a,) = torch.autograd.grad(w.dense_bias(), w.relative_position_bias_table, g)
    (b,) = torch.autograd.grad(t[flipped.reshape(-1)].reshape(49, 49, 3).permute(2, 0, 1), t, g)
    assert rel(a, b) < 1e-6


# ------------------------------------------------------------------------------------------------ constructor, state dict
def reference_backbone_cfg(name):
    return dict(type=name, embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7, mlp_ratio=4,
                qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.2, patch_norm=True,
                out_indices=[1, 2, 3], with_cp=False, convert_weights=True,
                init_cfg=dict(type="Pretrained", checkpoint="swin_tiny_patch4_window7_224.pth"))


@pytest.fixture(scope="module")
def backbone():
    torch.manual_seed(0)
    return MODELS.build(reference_backbone_cfg("mmdet.SwinTransformer")).eval()


def test_reference_config_builds_under_both_names(backbone):
    other = MODELS.build(reference_backbone_cfg("SwinTransformer"))
    assert type(other) is type(backbone) is swin.SwinTransformer
    assert backbone.convert_weights is True and backbone.init_cfg["type"] == "Pretrained"
    with torch.no_grad():
        outs = backbone(torch.randn(1, 3, 64, 96))
    assert [tuple(o.shape) for o in outs] == [(1, 192, 8, 12), (1, 384, 4, 6), (1, 768, 2, 3)]
    for o in outs:  # [B, C, H, W] views of [B, H, W, C] memory
        assert o.permute(0, 2, 3, 1).is_contiguous()


def expected_keys(depths=(2, 2, 6, 2), out_indices=(1, 2, 3)):
    wb = lambda p: [p + ".weight", p + ".bias"]  # noqa: E731
    keys = wb("patch_embed.projection") + wb("patch_embed.norm")
    for s, d in enumerate(depths):
        for b in range(d):
            p = "stages.%d.blocks.%d." % (s, b)
            keys += wb(p + "norm1") + wb(p + "norm2") + wb(p + "attn.w_msa.qkv") + wb(p + "attn.w_msa.proj")
            keys += [p + "attn.w_msa.relative_position_bias_table", p + "attn.w_msa.relative_position_index"]
            keys += wb(p + "ffn.layers.0.0") + wb(p + "ffn.layers.1")
        if s < len(depths) - 1:
            keys += wb("stages.%d.downsample.norm" % s) + ["stages.%d.downsample.reduction.weight" % s]
    for i in out_indices:
        keys += wb("norm%d" % i)
    return keys


def test_state_dict_keys_and_shapes(backbone):
    sd = backbone.state_dict()
    assert sorted(sd) == sorted(expected_keys())
    assert sd["stages.2.blocks.5.attn.w_msa.relative_position_bias_table"].shape == (169, 12)
    assert sd["stages.0.blocks.1.attn.w_msa.relative_position_index"].shape == (49, 49)
    assert sd["stages.1.blocks.0.attn.w_msa.qkv.weight"].shape == (576, 192)
    assert sd["stages.0.downsample.reduction.weight"].shape == (192, 384)
    assert sd["stages.3.blocks.0.ffn.layers.0.0.weight"].shape == (3072, 768)
    assert sd["patch_embed.projection.weight"].shape == (96, 3, 4, 4)
    assert [blk.attn.shift_size for blk in backbone.stages[2].blocks] == [0, 3, 0, 3, 0, 3]
    rates = [blk.drop_path_rate for st in backbone.stages for blk in st.blocks]
    assert rates[0] == 0.0 and abs(rates[-1] - 0.2) < 1e-12
    assert all(abs((b - a) - 0.2 / 11) < 1e-12 for a, b in zip(rates, rates[1:]))


def test_state_dict_round_trip_is_bit_exact(backbone):
    torch.manual_seed(1)
    other = MODELS.build(reference_backbone_cfg("SwinTransformer")).eval()
    other.load_state_dict(backbone.state_dict())
    x = torch.randn(2, 3, 64, 96)
    with torch.no_grad():
        for a, b in zip(backbone(x), other(x)):
            assert torch.equal(a, b)


def test_input_that_is_no_multiple_of_the_patch_is_padded(backbone):
    with torch.no_grad():
        outs = backbone(torch.randn(1, 3, 62, 90))
    assert [tuple(o.shape[2:]) for o in outs] == [(8, 12), (4, 6), (2, 3)]


def test_with_cp_gives_the_same_gradients():
    torch.manual_seed(2)
    cfg = dict(embed_dims=96, depths=[2, 2], num_heads=[3, 6], strides=(4, 2), out_indices=[0, 1], drop_path_rate=0.0)
    a = swin.SwinTransformer(**cfg).train()
    b = swin.SwinTransformer(with_cp=True, **cfg).train()
    b.load_state_dict(a.state_dict())
    x = torch.randn(1, 3, 32, 48, requires_grad=True)
    for m in (a, b):
        sum(o.square().mean() for o in m(x)).backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p.grad, q.grad, rtol=1e-5, atol=1e-8), n


# ------------------------------------------------------------------------------------------------ patch merging, drop path
def test_patch_merging_channel_order_is_unfold():
    x = torch.randn(2, 6, 10, 5)                                       # [B, H, W, C]
    want = torch.nn.Unfold(2, stride=2)(x.permute(0, 3, 1, 2))         # [B, 4C, L]
    got = swin.PatchMerging.gather(x)
    assert torch.equal(got.reshape(2, -1, 20), want.transpose(1, 2))
    odd = swin.PatchMerging.gather(torch.randn(1, 5, 7, 3))            # padded right / bottom
    assert odd.shape == (1, 3, 4, 12) and not odd[:, -1, :, 2::4].any() and not odd[:, :, -1, 1::2].any()


def test_drop_path():
    x = torch.randn(64, 3, 4, 5)
    assert swin.drop_path(x, 0.3, False) is x and swin.drop_path(x, 0.0, True) is x
    torch.manual_seed(0)
    y = swin.drop_path(x, 0.25, True)
    dropped = (y.reshape(64, -1) == 0).all(1)
    assert 0 < int(dropped.sum()) < 64
    assert torch.allclose(y[~dropped], x[~dropped] / 0.75)
    blk = swin.SwinBlock(96, 3, 384, drop_path_rate=0.5).eval()
    a = torch.randn(2, 7, 7, 96)
    with torch.no_grad():
        assert torch.equal(blk(a), blk(a))


# ------------------------------------------------------------------------------------------------ config, support query
def test_nuscenes_config_with_swin_builds_a_bevfusion():
    from bevfusion_amd.bevfusion import BEVFusion, nuscenes_config
    assert nuscenes_config()["img_backbone"] == dict(type="ResNet50")
    assert nuscenes_config()["img_neck"]["in_channels"] == [512, 1024, 2048]
    cfg = nuscenes_config(img_backbone="swin_t")
    want = reference_backbone_cfg("mmdet.SwinTransformer")
    assert cfg["img_backbone"] == want and cfg["img_neck"]["in_channels"] == [192, 384, 768]
    model = MODELS.build(cfg)
    assert isinstance(model, BEVFusion) and isinstance(model.img_backbone, swin.SwinTransformer)
    assert model.img_neck.lateral_convs[1].conv.in_channels == 384 + 768


def test_support_query_is_host_only():
    from bevfusion_amd import _lib
    ok = _lib.load().bfhip_swin_attn_supported  # (B, Hp, Wp, heads, window, head_dim, shift)
    assert ok(24, 70, 182, 3, 7, 32, 3) == 1 and ok(1, 7, 7, 24, 7, 32, 0) == 1
    assert ok(24, 70, 182, 3, 8, 32, 3) == 0       # window 8
    assert ok(24, 70, 182, 3, 7, 16, 3) == 0       # head dim 16
    assert ok(24, 64, 182, 3, 7, 32, 3) == 0       # Hp % 7 != 0
    assert ok(24, 70, 176, 3, 7, 32, 0) == 0       # Wp % 7 != 0
    assert ok(24, 70, 182, 3, 7, 32, 2) == 0       # a shift the mask regions are not built for
    parts = _lib.load().bfhip_swin_attn_parts
    assert parts(1, 7, 7, 6) == 1 and 0 < parts(24, 70, 182, 3) < 24 * 10 * 26
