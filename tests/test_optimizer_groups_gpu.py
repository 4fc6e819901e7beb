"""GPU: parameter groups, per-step schedules and checkpoint resume of amp.MasterWeightAdamW (csrc/optim.hip,
bfhip_adamw_step_groups).

The net is the one of test_model_gpu.test_optimizer_paths_agree_and_skip_nonfinite_steps plus a Linear(288, 16) placed right
after the first conv: its 4608 weights span two 4096-element chunks of the flat table, its weight sits between tensors of two
other groups (the first conv's bias; its own bias, alone in a group), so chunk -> tensor -> group indexing is exercised at the
smallest shapes where it can go wrong.  Gradients are handed to the optimizers directly; no forward pass is needed."""
import contextlib
import copy
import io
import math
import os
import warnings

import numpy as np
import pytest
import torch
from torch import nn

LR, WD, MAX_NORM, STEPS = 1e-2, 0.01, 0.5, 8
PATHS = {"flat": ("1", "1"), "direct": ("0", "1"), "object": ("0", "0")}
# four groups: the first conv at lr / 10, norms without weight decay, one that holds a single bias tensor, the rest
CFG = dict(custom_keys={"conv1": dict(lr_mult=0.1), "wide.bias": dict(decay_mult=0.5)}, norm_decay_mult=0.0)


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(8, 16, 3, padding=1)
        self.wide = nn.Linear(8 * 6 * 6, 16)
        self.bn = nn.BatchNorm2d(16)
        self.conv2 = nn.Conv2d(16, 8, 1)
        self.fc = nn.Linear(8 * 6 * 6, 5)


@contextlib.contextmanager
def _path(name):
    keys = ("BFHIP_FLAT_ADAMW", "BFHIP_DIRECT_ADAMW")
    old = [os.environ.get(k) for k in keys]
    os.environ.update(zip(keys, PATHS[name]))
    try:
        yield
    finally:
        for k, v in zip(keys, old):
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _make(base, path):
    from bevfusion_amd.amp import MasterWeightAdamW
    net = copy.deepcopy(base)
    with _path(path):
        mw = MasterWeightAdamW(net, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM, exclude=(), paramwise_cfg=CFG)
    assert (mw.flat, mw.direct) == (path == "flat", path == "direct")
    return net, mw


def _beta1(t):
    """The reference's momentum schedule (two CosineAnnealingMomentum phases, closed form eta_min + (base - eta_min) *
    (1 + cos(pi t / T)) / 2): 0.95 down to 0.85 over the first half of the run, back up to 0.95 over the second."""
    half = STEPS // 2
    if t < half:
        return 0.85 + (0.95 - 0.85) * (1 + math.cos(math.pi * t / half)) / 2
    return 0.95 + (0.85 - 0.95) * (1 + math.cos(math.pi * (t - half) / half)) / 2


class _Schedule:
    """LinearLR warm-up and CosineAnnealingLR on a torch optimizer, beta1 set by hand before every step; host work only."""

    def __init__(self, opt):
        self.opt = opt
        self.scheds = [torch.optim.lr_scheduler.LinearLR(opt, start_factor=1 / 3, total_iters=4),
                       torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=STEPS, eta_min=LR * 1e-4)]

    def before(self, t):
        for g in self.opt.param_groups:
            g["betas"] = (_beta1(t), g["betas"][1])

    def after(self):
        for s in self.scheds:
            s.step()

    def state_dict(self):
        return [s.state_dict() for s in self.scheds]

    def load_state_dict(self, states):
        for s, st in zip(self.scheds, states):
            s.load_state_dict(st)


def _run(net, mw, sched, grads, steps):
    for t in steps:
        mw.zero_grad()
        for p, g in zip(net.parameters(), grads[t]):
            p.grad = g.to(p.dtype).clone(memory_format=torch.preserve_format)
        sched.before(t)
        mw.step()
        sched.after()


def _moments(mw):
    if mw.flat:
        return mw._flat_m, mw._flat_v
    if mw.direct:
        return mw._exp_avg, mw._exp_avg_sq
    params = mw.master + mw.other
    return [mw.opt.state[p]["exp_avg"] for p in params], [mw.opt.state[p]["exp_avg_sq"] for p in params]


def _close(a, b, what):
    tol = 1e-5 if a.dtype == torch.float32 else 2 ** -7   # tests/test_model_gpu.py: flat path against torch
    assert torch.allclose(a.float(), b.float(), rtol=tol, atol=1e-7), (what, float((a.float() - b.float()).abs().max()))


@pytest.fixture(scope="module")
def case(dev):
    """The initial net, the gradients of every step and what torch computes from them: an fp32 copy under torch.optim.AdamW over
    the same groups with clip_grad_norm_, its gradients rounded to bf16 where the parameter is bf16 in MasterWeightAdamW."""
    from bevfusion_amd.amp import build_param_groups, low_precision_parameters
    torch.manual_seed(0)
    base = _Net().to(dev).to(memory_format=torch.channels_last)
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [[torch.randn(p.shape, generator=gen, device=dev) * (3.0 if t % 2 else 0.01) for p in base.parameters()]
             for t in range(STEPS)]
    ref = copy.deepcopy(base)
    low = {id(p) for p in low_precision_parameters(ref, exclude=())}
    named = dict(ref.named_parameters())
    groups = build_param_groups(ref, LR, WD, CFG)
    assert len(groups) == 4 and ["wide.bias"] in [names for _, names in groups]
    opt = torch.optim.AdamW([dict(params=[named[n] for n in names], **hyper) for hyper, names in groups], lr=LR, weight_decay=WD)
    sched = _Schedule(opt)
    for t in range(STEPS):
        for p, g in zip(ref.parameters(), grads[t]):
            p.grad = g.to(torch.bfloat16).float() if id(p) in low else g.clone()
        sched.before(t)
        torch.nn.utils.clip_grad_norm_(list(ref.parameters()), MAX_NORM)
        opt.step()
        sched.after()
    return dict(base=base, grads=grads, ref=ref, low=low, opt=opt)


def _raw_table(dev, seed):
    """A flat table as amp._build_flat lays it out, on plain tensors: (shape, bf16 copy and bf16 gradient?)."""
    from bevfusion_amd import _lib
    lib = _lib.load()
    shapes = [((16, 8, 3, 3), True), ((16,), False), ((16, 288), True), ((16,), True), ((5,), False)]
    gen = torch.Generator(device=dev).manual_seed(seed)
    t = dict(master=[torch.randn(s, generator=gen, device=dev) for s, _ in shapes])
    t["m"] = [torch.zeros_like(x) for x in t["master"]]
    t["v"] = [torch.zeros_like(x) for x in t["master"]]
    t["lowp"] = [x.to(torch.bfloat16) if low else None for x, (_, low) in zip(t["master"], shapes)]
    seg_dt = np.dtype([("master", "<u8"), ("m", "<u8"), ("v", "<u8"), ("lowp", "<u8"), ("n", "<i8"), ("grad_bf16", "<i4"),
                       ("group", "<i4")])
    assert seg_dt.itemsize == lib.bfhip_adamw_segment_bytes() == 48
    chunk = lib.bfhip_adamw_chunk_elems()
    segs, chunks = np.zeros(len(shapes), seg_dt), []
    for i, (x, m, v, lo) in enumerate(zip(t["master"], t["m"], t["v"], t["lowp"])):
        segs[i] = (x.data_ptr(), m.data_ptr(), v.data_ptr(), lo.data_ptr() if lo is not None else 0, x.numel(),
                   1 if lo is not None else 0, 0)
        chunks += [(i, c) for c in range(-(-x.numel() // chunk))]
    assert len(chunks) == len(shapes) + 1                        # the 4608-element tensor takes two
    t["segs"] = torch.from_numpy(segs.view(np.uint8).copy()).to(dev)
    t["chunks"] = torch.tensor(chunks, dtype=torch.int32, device=dev)
    t["partial"] = torch.empty(len(chunks), dtype=torch.float32, device=dev)
    t["scalars"] = torch.zeros(8, dtype=torch.float32, device=dev)
    t["grad_dtype"] = [torch.bfloat16 if low else torch.float32 for _, low in shapes]
    return t


@pytest.mark.gpu
def test_one_group_is_bit_identical_to_the_by_value_entry(dev):
    """The yardstick: the same table driven through bfhip_adamw_step (hyper-parameters by value) and through
    bfhip_adamw_step_groups with one group gives the same bits in masters, both moments, bf16 copies and scalars[0:6] after every
    one of 5 steps -- a clipped step, an unclipped one, a NaN gradient (step 3: nothing changes), a missing gradient (step 4)."""
    from bevfusion_amd import _lib
    a, b = _raw_table(dev, 7), _raw_table(dev, 7)
    gen = torch.Generator(device=dev).manual_seed(2)
    stream = _lib.stream_of(a["segs"])
    for step in range(5):
        grads = [(torch.randn(x.shape, generator=gen, device=dev) * (3.0 if step % 2 else 0.01)).to(dt)
                 for x, dt in zip(a["master"], a["grad_dtype"])]
        if step == 3:
            grads[0][0, 0, 0, 0] = float("nan")
        if step == 4:
            grads[2] = None
        ptrs = torch.tensor([0 if g is None else g.data_ptr() for g in grads], dtype=torch.int64, device=dev)
        lr, b1, b2, eps, wd = 1e-2 * (step + 1) / 3, _beta1(step), 0.99, 1e-8, 0.01
        before = [x.clone() for x in b["master"]]
        _lib.call("bfhip_adamw_step", a["segs"].data_ptr(), ptrs.data_ptr(), a["chunks"].data_ptr(), len(a["chunks"]),
                  a["partial"].data_ptr(), a["scalars"].data_ptr(), lr, b1, b2, eps, wd, MAX_NORM, stream)
        host = np.array([[lr, b1, b2, eps, wd, 0, 0, 0]], np.float32)
        groups = torch.from_numpy(host).to(dev)
        _lib.call("bfhip_adamw_step_groups", b["segs"].data_ptr(), ptrs.data_ptr(), b["chunks"].data_ptr(), len(b["chunks"]),
                  b["partial"].data_ptr(), b["scalars"].data_ptr(), groups.data_ptr(), host.ctypes.data, 1, MAX_NORM, stream)
        torch.cuda.synchronize()
        for key in ("master", "m", "v", "lowp"):
            for i, (x, y) in enumerate(zip(a[key], b[key])):
                assert (x is None and y is None) or torch.equal(x, y), (step, key, i)
        # as bit patterns: at step 3 the clip scale and the norm are NaN in both, and NaN != NaN
        assert torch.equal(a["scalars"][:6].view(torch.int32), b["scalars"][:6].view(torch.int32)), (step, a["scalars"], b["scalars"])
        assert float(b["scalars"][6]) == 0.0                    # every tensor named an existing group
        assert float(b["scalars"][1]) == (1.0 if step == 3 else 0.0)
        changed = any(not torch.equal(x, y) for x, y in zip(before, b["master"]))
        assert changed == (step != 3), step
        assert torch.equal(groups[0, 5:7], b["scalars"][3:5])  # the group's bias corrections, written on the device
    assert float(b["scalars"][2]) == 4.0


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_groups_and_per_step_schedules_match_torch(case, path):
    """Four groups from paramwise_cfg, lr warmed up and annealed by torch schedulers built on mw.opt, beta1 set every step: after 8
    steps queued without a host read in between (the host runs ahead of the device: what the pinned-image guard is for), every
    path agrees with torch.optim.AdamW over the same groups.  Before this feature the flat and direct paths kept the constructor's
    lr (3x the warmed-up one at step 1)."""
    net, mw = _make(case["base"], path)
    assert len(mw.param_groups) == 4 and mw.param_groups is mw.opt.param_groups
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        sched = _Schedule(mw.opt)
        _run(net, mw, sched, case["grads"], range(STEPS))
    order = [str(w.message) for w in caught if "optimizer.step()" in str(w.message)]
    assert not order, order                                     # the schedulers saw the optimizer step before they did
    ref = list(case["ref"].parameters())
    masters = {id(p): m for p, m in zip(mw.low, mw.master)}
    for (name, p), r in zip(net.named_parameters(), ref):
        assert (id(p) in masters) == (id(r) in case["low"]), name
        if id(p) in masters:
            assert p.dtype == torch.bfloat16
            _close(masters[id(p)], r, name + " (master)")
        _close(p.detach(), r.detach(), name)
    assert [g["lr"] for g in mw.param_groups] == [g["lr"] for g in case["opt"].param_groups]   # the same host arithmetic
    if mw.flat:
        assert float(mw.scalars[2]) == STEPS and float(mw.scalars[6]) == 0.0


def _resume(case, first, second):
    """3 steps on path `first`, checkpoint through torch.save / torch.load(map_location="cpu"), 3 more on path `second` in a
    fresh net and optimizer."""
    net, mw = _make(case["base"], first)
    sched = _Schedule(mw.opt)
    _run(net, mw, sched, case["grads"], range(3))
    buf = io.BytesIO()
    torch.save(dict(model=net.state_dict(), opt=mw.state_dict(), sched=sched.state_dict()), buf)
    buf.seek(0)
    ckpt = torch.load(buf, map_location="cpu")
    assert all(not t.is_cuda for s in ckpt["opt"]["state"].values() for t in s.values()) and not ckpt["opt"]["master"][0].is_cuda
    net2, mw2 = _make(case["base"], second)
    sched2 = _Schedule(mw2.opt)
    net2.load_state_dict(ckpt["model"])
    ptrs = [t.data_ptr() for t in mw2.master] + ([t.data_ptr() for lst in _moments(mw2) for t in lst] if second != "object" else [])
    groups = mw2.param_groups
    mw2.load_state_dict(ckpt["opt"])
    sched2.load_state_dict(ckpt["sched"])
    assert ptrs == [t.data_ptr() for t in mw2.master] + ([t.data_ptr() for lst in _moments(mw2) for t in lst] if second != "object" else [])
    assert mw2.param_groups is groups and mw2.opt.param_groups is groups
    assert [g["lr"] for g in groups] == [g["lr"] for g in mw.param_groups]
    for p, m in zip(mw2.low, mw2.master):
        assert torch.equal(p.detach(), m.to(torch.bfloat16))      # the bf16 parameters were refreshed from the masters
    _run(net2, mw2, sched2, case["grads"], range(3, 6))
    return net2, mw2


@pytest.mark.gpu
def test_resume_from_a_checkpoint_repeats_the_straight_run_bit_for_bit(case):
    """Flat path: 3 steps + state_dict + torch.save / load on the CPU + load_state_dict into a fresh optimizer + 3 steps equals 6
    steps straight in every bit of masters, moments, bf16 parameters and the step counter; load_state_dict copies in place (the
    flat tables keep pointing at the same masters and moments).  Before this feature there was no state_dict."""
    net, mw = _make(case["base"], "flat")
    _run(net, mw, _Schedule(mw.opt), case["grads"], range(6))
    net2, mw2 = _resume(case, "flat", "flat")
    for key, (xs, ys) in dict(master=(mw.master, mw2.master), m=(mw._flat_m, mw2._flat_m), v=(mw._flat_v, mw2._flat_v),
                              param=(list(net.parameters()), list(net2.parameters()))).items():
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(x, y), (key, i)
    assert float(mw2.scalars[2]) == float(mw.scalars[2]) == 6.0
    for (n, x), (_, y) in zip(net.named_buffers(), net2.named_buffers()):
        assert torch.equal(x, y), n


@pytest.mark.gpu
@pytest.mark.parametrize("first,second", [("flat", "object"), ("object", "flat")])
def test_a_state_written_by_one_path_loads_into_another(case, first, second):
    """The state layout does not depend on the path that wrote it: 3 steps on one path, 3 more on the other after a load, agree
    with 6 steps straight on the flat path within the flat-against-torch tolerances."""
    net, mw = _make(case["base"], "flat")
    _run(net, mw, _Schedule(mw.opt), case["grads"], range(6))
    net2, mw2 = _resume(case, first, second)
    for i, (x, y) in enumerate(zip(mw.master, mw2.master)):
        _close(x, y, "master %d" % i)
    for (n, x), (_, y) in zip(net.named_parameters(), net2.named_parameters()):
        _close(x.detach(), y.detach(), n)
    step = float(mw2.scalars[2]) if mw2.flat else float(mw2.opt.state[mw2.master[0]]["step"])
    assert step == 6.0


@pytest.mark.gpu
def test_unequal_steps_and_bad_group_hyper_parameters_are_errors(case):
    from bevfusion_amd import _lib
    net, mw = _make(case["base"], "flat")
    sd = mw.state_dict()
    assert sorted(sd) == ["master", "param_groups", "state"] and len(sd["state"]) == len(mw.master) + len(mw.other)
    sd["state"][1]["step"] = torch.tensor(2.0)
    with pytest.raises(ValueError, match="one step counter"):
        mw.load_state_dict(sd)
    for p, g in zip(net.parameters(), case["grads"][0]):
        p.grad = g.to(p.dtype)
    mw.param_groups[2]["betas"] = (1.0, 0.999)
    before = [m.clone() for m in mw.master]
    with pytest.raises(RuntimeError, match="group 2"):
        mw.step()
    assert "group 2" in _lib.load().bfhip_last_error().decode()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, mw.master)) and float(mw.scalars[2]) == 0.0   # nothing was launched
    mw.param_groups[2]["betas"] = (0.9, 0.999)
    mw.step()
    torch.cuda.synchronize()
    assert float(mw.scalars[2]) == 1.0 and not torch.equal(before[0], mw.master[0])
