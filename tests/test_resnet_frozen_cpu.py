"""CPU: `frozen_stages` and `norm_eval` of the ResNet-50 backbone (mmdet 3.x's `_freeze_stages` and `train()`, written from
knowledge of that package: parity unpinned, like tests/test_swin_frozen_cpu.py)."""
import copy

import torch
from torch import nn

import bevfusion_amd  # noqa: F401
from bevfusion_amd.dense_modules import ResNet50

FROZEN1 = ("conv1.", "bn1.", "layer1.")
_BN = nn.modules.batchnorm._BatchNorm


def build(**kw):
    torch.manual_seed(0)
    return ResNet50(**kw)


def check_frozen1_norm_eval(net):
    assert net.training
    for m in (net.conv1, net.bn1, net.layer1):
        assert all(not c.training for c in m.modules())
    assert all(not m.training for m in net.modules() if isinstance(m, _BN))
    for layer in (net.layer2, net.layer3, net.layer4):
        convs = [m for m in layer.modules() if isinstance(m, nn.Conv2d)]
        assert convs and all(m.training for m in convs)
    for n, p in net.named_parameters():
        assert p.requires_grad == (not n.startswith(FROZEN1)), n
    assert net.layer2[0].bn1.weight.requires_grad and net.layer4[2].bn3.bias.requires_grad


def test_frozen_stem_and_layer1_with_norm_eval():
    net = build(frozen_stages=1, norm_eval=True).train()
    check_frozen1_norm_eval(net)
    net.eval()
    assert not any(c.training for c in net.modules())
    net.train()
    check_frozen1_norm_eval(net)


def test_frozen_stages_zero_freezes_the_stem_alone():
    net = build(frozen_stages=0).train()
    assert not net.conv1.training and not net.bn1.training
    assert all(c.training for c in net.layer1.modules())
    assert all(m.training for m in net.layer2.modules() if isinstance(m, _BN))  # norm_eval is off
    frozen = [n for n, p in net.named_parameters() if not p.requires_grad]
    assert frozen == [n for n, _ in net.named_parameters() if n.startswith(("conv1.", "bn1."))]


def test_defaults_freeze_nothing():
    net = build().train()
    assert net.frozen_stages == -1 and net.norm_eval is False
    assert all(c.training for c in net.modules())
    assert all(p.requires_grad for p in net.parameters())


def test_state_dict_keys_do_not_depend_on_the_arguments():
    keys = list(build().state_dict())
    for kw in (dict(frozen_stages=0), dict(frozen_stages=1, norm_eval=True), dict(norm_eval=True), dict(frozen_stages=4)):
        assert list(build(**kw).state_dict()) == keys, kw


def test_forward_backward_matches_a_default_net_with_its_norms_in_eval():
    frozen = build(frozen_stages=1, norm_eval=True).train()
    with torch.no_grad():  # running statistics away from the (0, 1) they start at
        g = torch.Generator().manual_seed(1)
        for m in frozen.modules():
            if isinstance(m, _BN):
                m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    free = build().train()
    free.load_state_dict(copy.deepcopy(frozen.state_dict()))
    for m in free.modules():
        if isinstance(m, _BN):
            m.eval()
    x = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(2))
    a, b = frozen(x), free(x)
    assert len(a) == 3 and [tuple(t.shape) for t in a] == [(1, 512, 8, 12), (1, 1024, 4, 6), (1, 2048, 2, 3)]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    sum(o.square().mean() for o in a).backward()
    for n, p in frozen.named_parameters():
        if n.startswith(FROZEN1):
            assert p.grad is None, n
        else:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
