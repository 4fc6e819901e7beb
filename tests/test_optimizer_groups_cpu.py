"""CPU: amp.build_param_groups, the rule that sorts a model's trainable parameters into optimizer groups (the subset of mmengine's
paramwise_cfg that BEVFusion recipes use: custom_keys, norm_decay_mult, bias_decay_mult).  Pure Python over module types and names."""
import pytest
import torch
from torch import nn

from bevfusion_amd.amp import build_param_groups

LR, WD = 1e-2, 0.05


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(4, 4, 3, padding=1)
        self.bn = nn.BatchNorm2d(4)


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = nn.ModuleDict(dict(stem=nn.Conv2d(3, 4, 3), layer1=nn.Sequential(_Block(), _Block())))
        self.neck = nn.Sequential(nn.Conv2d(4, 4, 1, bias=False), nn.LayerNorm(4))
        self.head = nn.Linear(4, 2)


def _as_dict(groups):
    return {n: (h["lr"], h["weight_decay"]) for h, names in groups for n in names}


def test_no_paramwise_cfg_is_one_group_in_parameter_order():
    net = _Net()
    for cfg in (None, {}):
        groups = build_param_groups(net, LR, WD, cfg)
        assert len(groups) == 1
        hyper, names = groups[0]
        assert hyper == dict(lr=LR, weight_decay=WD)
        assert names == [n for n, _ in net.named_parameters()]


def test_norm_and_bias_decay_multipliers():
    net = _Net()
    got = _as_dict(build_param_groups(net, LR, WD, dict(norm_decay_mult=0.0, bias_decay_mult=0.0)))
    for name in got:
        norm = ".bn." in name or name.startswith("neck.1.")
        assert got[name] == (LR, 0.0 if norm or name.endswith(".bias") else WD), name
    # each rule on its own: a norm's bias is a norm parameter, not a `bias` of the bias rule
    got = _as_dict(build_param_groups(net, LR, WD, dict(bias_decay_mult=0.5)))
    assert got["backbone.layer1.0.bn.bias"] == (LR, WD) and got["neck.1.bias"] == (LR, WD)
    assert got["backbone.stem.bias"] == (LR, 0.5 * WD) and got["head.bias"] == (LR, 0.5 * WD)
    assert got["backbone.stem.weight"] == (LR, WD)
    got = _as_dict(build_param_groups(net, LR, WD, dict(norm_decay_mult=0.25)))
    assert got["backbone.layer1.1.bn.weight"] == (LR, 0.25 * WD) and got["neck.1.bias"] == (LR, 0.25 * WD)
    assert got["head.bias"] == (LR, WD)


def test_custom_keys_longest_key_wins_and_overrides_the_mult_rules():
    net = _Net()
    cfg = dict(custom_keys={"backbone": dict(lr_mult=0.1), "backbone.layer1.1": dict(lr_mult=0.5, decay_mult=2.0),
                            "head.bias": dict(decay_mult=3.0)},
               norm_decay_mult=0.0, bias_decay_mult=0.0)
    got = _as_dict(build_param_groups(net, LR, WD, cfg))
    assert got["backbone.stem.weight"] == (LR * 0.1, WD)
    assert got["backbone.stem.bias"] == (LR * 0.1, WD)                 # a custom key beats bias_decay_mult (decay_mult defaults to 1)
    assert got["backbone.layer1.0.bn.weight"] == (LR * 0.1, WD)        # ... and norm_decay_mult
    assert got["backbone.layer1.1.conv.weight"] == (LR * 0.5, WD * 2.0)  # the longer of two matching keys
    assert got["backbone.layer1.1.bn.bias"] == (LR * 0.5, WD * 2.0)
    assert got["head.bias"] == (LR, WD * 3.0)
    assert got["head.weight"] == (LR, WD)
    assert got["neck.1.weight"] == (LR, 0.0) and got["neck.0.weight"] == (LR, WD)


def test_custom_keys_of_equal_length_break_ties_alphabetically():
    net = _Net()
    for keys in (("neck.0", "0.weig"), ("0.weig", "neck.0")):   # both occur in "neck.0.weight"; insertion order must not matter
        cfg = dict(custom_keys={k: dict(lr_mult=2.0 if k == "0.weig" else 4.0) for k in keys})
        got = _as_dict(build_param_groups(net, LR, WD, cfg))
        assert got["neck.0.weight"] == (LR * 2.0, WD)


def test_equal_hyper_parameters_merge_in_first_seen_order_and_cover_every_trainable_parameter_once():
    net = _Net()
    net.backbone["stem"].weight.requires_grad_(False)               # a frozen parameter is in no group
    net.alias = net.head                                             # a module reachable under two names is grouped once
    cfg = dict(custom_keys={"backbone": dict(lr_mult=0.1)}, norm_decay_mult=0.0, bias_decay_mult=0.0)
    groups = build_param_groups(net, LR, WD, cfg)
    assert [h for h, _ in groups] == [dict(lr=LR * 0.1, weight_decay=WD), dict(lr=LR, weight_decay=WD),
                                      dict(lr=LR, weight_decay=0.0)]   # backbone first, neck.0.weight, then neck.1.* + head.bias
    assert groups[2][1] == ["neck.1.weight", "neck.1.bias", "head.bias"]
    assert groups[1][1] == ["neck.0.weight", "head.weight"]
    names = [n for _, ns in groups for n in ns]
    want = [n for n, p in net.named_parameters() if p.requires_grad]
    assert sorted(names) == sorted(want) and len(set(names)) == len(names)
    assert "backbone.stem.weight" not in names
    assert len(groups) < len(names)                                  # not one group per parameter
    assert build_param_groups(net, LR, WD, cfg) == groups            # stable from call to call
    pos = {n: i for i, n in enumerate(want)}
    for _, ns in groups:
        assert [pos[n] for n in ns] == sorted(pos[n] for n in ns)    # inside a group: the model's parameter order


def test_unknown_keys_are_an_error():
    net = _Net()
    with pytest.raises(ValueError, match="bias_lr_mult"):
        build_param_groups(net, LR, WD, dict(bias_lr_mult=2.0))
    with pytest.raises(ValueError, match="momentum"):
        build_param_groups(net, LR, WD, dict(custom_keys={"head": dict(momentum=0.5)}))


def test_optimizer_groups_on_the_cpu_follow_the_rule():
    """MasterWeightAdamW builds self.opt with these groups; self.param_groups is that optimizer's own list."""
    from bevfusion_amd.amp import MasterWeightAdamW
    torch.manual_seed(0)
    net = _Net()
    cfg = dict(custom_keys={"backbone": dict(lr_mult=0.1)}, norm_decay_mult=0.0)
    mw = MasterWeightAdamW(net, lr=LR, weight_decay=WD, max_grad_norm=1.0, exclude=(), betas=(0.8, 0.9), eps=1e-6, paramwise_cfg=cfg)
    assert mw.param_groups is mw.opt.param_groups and not mw.flat
    want = build_param_groups(net, LR, WD, cfg)
    assert [(g["lr"], g["weight_decay"], len(g["params"])) for g in mw.param_groups] == [
        (h["lr"], h["weight_decay"], len(ns)) for h, ns in want]
    assert all(g["betas"] == (0.8, 0.9) and g["eps"] == 1e-6 for g in mw.param_groups)
    assert sum(len(g["params"]) for g in mw.param_groups) == len(mw.master) + len(mw.other)
