"""CPU: `frozen_stages` of the Swin backbone (mmdet 3.x's `_freeze_stages`, written from knowledge of that package: parity
unpinned like the rest of bevfusion_amd/swin.py), and the CPU behaviour of bevfusion_amd/layernorm.py (plain torch, exactly)."""
import copy

import torch
import torch.nn.functional as F

import bevfusion_amd  # noqa: F401
from bevfusion_amd import layernorm, swin

CFG = dict(embed_dims=96, depths=[1, 1, 1, 1], num_heads=[3, 6, 12, 24], out_indices=[1, 2, 3], drop_path_rate=0.0)
FROZEN = ("patch_embed.", "stages.0.", "stages.1.", "norm1.")


def build(frozen):
    torch.manual_seed(0)
    return swin.SwinTransformer(frozen_stages=frozen, **CFG)


def test_frozen_parts_stay_in_eval_and_without_grad():
    net = build(2).train()
    for m in (net.patch_embed, net.drop_after_pos, net.stages[0], net.stages[1], net.norm1):
        assert all(not c.training for c in m.modules())
    for m in (net.stages[2], net.stages[3], net.norm2, net.norm3):
        assert all(c.training for c in m.modules())
    assert net.training
    for n, p in net.named_parameters():
        assert p.requires_grad == (not n.startswith(FROZEN)), n
    assert any(n.startswith("stages.1.downsample.") for n, p in net.named_parameters() if not p.requires_grad)
    net.eval()
    assert not any(c.training for c in net.modules())
    net.train()
    assert not net.stages[1].training and net.stages[2].training
    # frozen_stages = 0 freezes the patch embedding alone; -1 nothing
    n0 = build(0).train()
    assert not n0.patch_embed.training and n0.stages[0].training
    assert [n for n, p in n0.named_parameters() if not p.requires_grad] == [n for n, _ in n0.named_parameters() if n.startswith("patch_embed.")]
    assert all(p.requires_grad for p in build(-1).parameters())


def test_frozen_outputs_grads_and_keys():
    frozen, free = build(2).train(), build(-1).train()
    assert list(frozen.state_dict()) == list(free.state_dict())
    free.load_state_dict(copy.deepcopy(frozen.state_dict()))
    x = torch.randn(1, 3, 56, 84)
    a, b = frozen(x), free(x)
    assert len(a) == 3
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    sum(o.square().mean() for o in a).backward()
    for n, p in frozen.named_parameters():
        if n.startswith(FROZEN):
            assert p.grad is None, n
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_layernorm_functions_on_the_cpu_are_plain_torch():
    torch.manual_seed(0)
    x, br = torch.randn(2, 5, 7, 96), torch.randn(2, 5, 7, 96)
    w, b = torch.rand(96) + 0.5, torch.randn(96)
    scale = torch.tensor([0.0, 1.25])
    before = dict(layernorm.LAUNCHES)
    assert torch.equal(layernorm.layer_norm_rows(x, w, b, 1e-5), F.layer_norm(x, (96,), w, b, 1e-5))
    assert layernorm.layer_norm_rows(x, w, b, 1e-5, torch.bfloat16).dtype == torch.bfloat16
    s = x + br * scale.view(2, 1, 1, 1)
    got_s, got_y = layernorm.add_layer_norm_rows(x, br, scale, w, b, 1e-5)
    assert torch.equal(got_s, s) and torch.equal(got_y, F.layer_norm(s, (96,), w, b, 1e-5))
    assert torch.equal(layernorm.scaled_add_rows(x, br, scale), s)
    assert torch.equal(layernorm.scaled_add_rows(x, br), x + br)
    assert layernorm.LAUNCHES == before


def test_drop_path_scale_draws_what_drop_path_draws():
    x = torch.randn(64, 3, 5)
    torch.manual_seed(3)
    want = swin.drop_path(x, 0.25, True)
    torch.manual_seed(3)
    scale = swin.drop_path_scale(x, 0.25, True)
    assert scale.shape == (64,) and scale.dtype == torch.float32 and 0 < int((scale == 0).sum()) < 64
    assert torch.equal(x * scale.view(-1, 1, 1), want)
    assert swin.drop_path_scale(x, 0.25, False) is None and swin.drop_path_scale(x, 0.0, True) is None


def test_block_on_the_cpu_is_unchanged_by_the_switch(monkeypatch):
    torch.manual_seed(0)
    blk = swin.SwinBlock(96, 3, 384, drop_path_rate=0.5).train()
    x = torch.randn(2, 7, 14, 96)
    outs = []
    for on in (True, False):
        monkeypatch.setattr(layernorm, "ENABLED", on)
        torch.manual_seed(1)
        outs.append(blk(x))
    assert torch.equal(*outs)
