"""GPU: the ASSEMBLED ResNet-50 trunk in training mode -- `dense_modules.ResNet50().layerK[:2]` (the projection / down-sampling
bottleneck followed by one identity bottleneck, so the second block's fork receives the fused BN + residual + ReLU output of the
first) under bf16 autocast on the MI355X, against the twin of tests/resnet_twin.py.

What is wired together here and nowhere else in the suite: `Conv2dHipWgrad.forward_fork` (identity / even-pixel fork, the skip
gradient added in conv1's data-gradient epilogue), `forward_unstrided` (the stride-2 shortcut on the subsampled input), the
statistics hand-over `_bfhip_stat_partial` -> `bfhip_bn2d_fwd_partials[_mask]`, bn3's bit mask, the per-layer choice of HIP or
library kernels, the grouped weight gradients and the transposed-weight cache.

Shapes (`resnet_twin.CASES`): the smallest that take the HIP paths -- output maps of 2 x 23 x 47 = 2162 >= conv2d.MIN_PIXELS pixels
with odd extents, one even-sized case on layer2 (44 x 96 -> 22 x 48: the 44 x 92 one would have 2024 output pixels and send the
second block to the library).

Every case asserts
  1. the PATH: the multiset of convolution / BatchNorm entry points that went through `_lib.call` (Python front-end) equals the one
     derived here from the `_resnet_conv` table -- a silent fall-back to the library fails; with the C++ front-end nothing goes
     through ctypes and no weight gradient is left queued;
  2. PARITY with the fp64 rounding twin over two training steps: every metric of `resnet_twin.measure` <= margin x its noise floor
     (3 global, 2.5 profile maxima; floors: the twin in fp32 against itself in fp64, computed from the reference alone), under the
     project's bf16 caps (forward relative L2 <= 1e-2 sqrt(7 convolutions), gradients cos >= 0.98 and relative L2 <= 0.2), and
     num_batches_tracked == 2;
further tests: the two front-ends bit for bit, the fork switches, norm_eval, and fp32 without autocast.

Not here: the comparison with torch's own autocast path on the GPU (`_RESNET_CONV = "lib"`, bn2d.FUSED_BN2D = False).  Its first
run ended in a segmentation fault of the host process inside torch's training-mode F.batch_norm on a bf16 channels-last map
(library code, never run by this suite before); the cause could not be read from this repository, so the test was taken out.

Measured on the MI355X (first run; worst step / worst parameter per family, same columns as the floors table of resnet_twin.py;
the bound of a column is 3 x (l2, gw, gbn, rm, rv) or 2.5 x (row, col, img, ch8) its floor):
case / mode                        out.l2  out.row  out.col  out.img  out.ch8   gin.l2  gin.row  gin.col  gin.img  gin.ch8    gw.l2   gbn.l2       rm       rv
K1      tuned = hip               1.3e-03  1.6e-03  1.8e-03  1.3e-03  1.6e-03  1.9e-02  3.1e-02  4.2e-02  2.2e-02  1.9e-02  2.2e-02  2.2e-02  3.5e-06  3.4e-06
K2      tuned = hip               2.9e-03  3.1e-03  3.3e-03  2.9e-03  3.4e-03  4.0e-02  4.7e-02  6.1e-02  4.1e-02  4.0e-02  4.3e-02  5.0e-02  6.8e-06  7.4e-06
K2even  tuned = hip               2.7e-03  2.9e-03  3.0e-03  2.7e-03  3.1e-03  4.0e-02  4.6e-02  5.8e-02  4.1e-02  4.1e-02  4.4e-02  5.2e-02  7.9e-06  7.7e-06
K3      tuned = hip               3.1e-03  3.2e-03  3.3e-03  3.1e-03  3.6e-03  4.5e-02  5.5e-02  5.8e-02  4.6e-02  4.6e-02  5.0e-02  5.4e-02  9.8e-06  9.3e-06
K4      tuned (worst of 4)        3.6e-03  3.8e-03  3.9e-03  3.7e-03  4.2e-03  5.5e-02  6.0e-02  7.7e-02  5.7e-02  5.6e-02  6.1e-02  7.2e-02  1.2e-05  1.5e-05
K4      hip                       3.3e-03  3.4e-03  3.6e-03  3.3e-03  3.8e-03  4.8e-02  5.2e-02  5.9e-02  4.9e-02  4.9e-02  5.4e-02  6.4e-02  1.3e-05  1.1e-05
K2      tuned, either fork off    2.9e-03  3.1e-03  3.3e-03  2.9e-03  3.4e-03  4.0e-02  4.9e-02  6.0e-02  4.1e-02  4.1e-02  4.4e-02  5.1e-02  8.0e-06  6.5e-06
K3      tuned, either fork off    3.1e-03  3.2e-03  3.4e-03  3.1e-03  3.7e-03  4.7e-02  5.6e-02  6.6e-02  4.7e-02  4.8e-02  5.2e-02  6.3e-02  1.1e-05  1.1e-05
K4      tuned, either fork off    3.6e-03  3.8e-03  3.9e-03  3.6e-03  4.2e-03  5.4e-02  5.9e-02  6.3e-02  5.5e-02  5.4e-02  6.0e-02  7.2e-02  1.1e-05  1.4e-05
K2      norm_eval, tuned = hip    2.2e-04  4.1e-04  5.3e-04  2.6e-04  3.5e-04  2.8e-03  8.4e-03  1.2e-02  3.1e-03  3.0e-03  8.1e-03  6.5e-03  0.0e+00  0.0e+00
  its floors (computed in the test) 2.2e-04  4.1e-04  5.3e-04  2.5e-04  3.3e-04  3.3e-03  1.7e-02  2.5e-02  4.2e-03  3.9e-03  7.8e-03  7.7e-03  0.0e+00  0.0e+00
K2      fp32, no autocast         forward max-norm 5.5e-07 / 5.8e-07 (bound 1e-3); input gradient relative L2 6.0e-07, all elements inside
(cached / uncached transposed weights and both front-ends give the same figures to the digits shown, except layer4 "tuned", whose
512-channel 3x3 forwards are the library's and differ from run to run in the last digit; K1 and K2even with a fork off equal
their forked rows / lie within 8 % of them.  Every figure lies between 0.8 x and 1.35 x its floor: the GPU is as close to the fp64
twin as the twin's own fp32 run is.  No margin was exceeded on the first run, so no rounding point was added after it.)
"""
import collections

import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib
from bevfusion_amd import bn2d
from bevfusion_amd import conv2d as c2
from bevfusion_amd import dense_modules as dm

import resnet_twin as rt

pytestmark = pytest.mark.gpu

CONV_AND_BN = ("bfhip_conv2d_fwd", "bfhip_conv2d_dgrad_wt", "bfhip_conv2d_dgrad", "bfhip_bn2d_fwd_partials",
               "bfhip_bn2d_fwd_partials_mask", "bfhip_bn2d_fwd", "bfhip_bn2d_bwd_mask", "bfhip_bn2d_bwd", "bfhip_conv2d_wgrad",
               "bfhip_conv2d_wgrad_group_launch")
N_CONVS = 7
STEPS = 2
_RUNS = {}


# ------------------------------------------------------------------------------------------ the `_resnet_conv` table, restated
def _choice(mode, k, stride, cin):
    """(forward on HIP, data gradient on HIP) of one trunk convolution as the comment above dense_modules._resnet_conv states it."""
    if mode == "hip":
        return True, True
    assert mode == "tuned"
    if k == 1 and stride == 1:
        return True, True
    if k == 3:
        return cin <= 256, True
    return False, False          # a stride-2 1x1 shortcut called as a plain layer (it normally runs through forward_unstrided)


def _layers(name, mode, forked):
    """[(state-dict name, N, H, W, Cin, Cout, k, stride, pad, hip forward, hip data gradient, BatchNorm adds a residual)]"""
    k, n, h, w = rt.CASES[name]
    inplanes, planes, stride = rt.STAGES[k]
    oh, ow = rt.out_hw(k, h, w)
    rows = []
    for b, (cin, s, ih, iw) in enumerate(((inplanes, stride, h, w), (planes * 4, 1, oh, ow))):
        rows.append(("%d.conv1" % b, n, ih, iw, cin, planes, 1, 1, 0) + _choice(mode, 1, 1, cin) + (False,))
        rows.append(("%d.conv2" % b, n, ih, iw, planes, planes, 3, s, 1) + _choice(mode, 3, s, planes) + (False,))
        rows.append(("%d.conv3" % b, n, oh, ow, planes, planes * 4, 1, 1, 0) + _choice(mode, 1, 1, planes) + (True,))
        if b == 0:
            if mode == "tuned" and s == 2 and forked:   # forward_unstrided: a stride-1 pointwise layer on the even pixels, all HIP
                rows.append(("0.downsample.0", n, oh, ow, cin, planes * 4, 1, 1, 0, True, True, False))
            else:
                rows.append(("0.downsample.0", n, ih, iw, cin, planes * 4, 1, s, 0) + _choice(mode, 1, s, cin) + (False,))
    return rows


def _expected_calls(name, mode, cached, forked):
    lib = _lib.load()
    c = collections.Counter()
    for (_, n, h, w, cin, cout, k, s, p, hip_fwd, hip_dgrad, residual) in _layers(name, mode, forked):
        assert lib.bfhip_conv2d_supported(n, h, w, cin, cout, k, k, s, p, 1) and n * h * w >= c2.MIN_PIXELS, (name, cin, cout, k, s)
        if hip_fwd:
            c["bfhip_conv2d_fwd"] += 1
            c["bfhip_bn2d_fwd_partials_mask" if residual else "bfhip_bn2d_fwd_partials"] += 1
        else:
            c["bfhip_bn2d_fwd"] += 1
        c["bfhip_bn2d_bwd_mask" if (hip_fwd and residual) else "bfhip_bn2d_bwd"] += 1
        if hip_dgrad:
            c["bfhip_conv2d_dgrad_wt" if cached else "bfhip_conv2d_dgrad"] += 1
        if not lib.bfhip_conv2d_wgrad_groupable(n, h, w, cin, cout, k, k, s, p, 1):
            c["bfhip_conv2d_wgrad"] += 1
    c["bfhip_conv2d_wgrad_group_launch"] = 1
    return collections.Counter({k: v * STEPS for k, v in c.items()})


def _lib_fwd(name, mode, forked):
    """The convolutions whose BatchNorm takes its statistics from the bf16 tensor (library forward: no partial sums handed over)."""
    return frozenset(r[0] for r in _layers(name, mode, forked) if not r[9])


# ------------------------------------------------------------------------------------------ one run of the product on the GPU
def _run(dev, name, mode, cached=True, front="ext", fork=True, shortcut_fork=True, norm_eval=False, fp32=False):
    """Two training steps of the product's layerK[:2]; memoised (results are CPU tensors and are never modified)."""
    key = (name, mode, cached, front, fork, shortcut_fork, norm_eval, fp32)
    if key in _RUNS:
        return _RUNS[key]
    k, n, h, w = rt.CASES[name]
    ext = _lib.torch_ext()
    if front == "ext" and (ext is None or not hasattr(ext, "conv2d")):
        pytest.fail("bfhip_torch_ext.so is missing or stale: the C++ front-end must be built in-tree")
    calls = []
    orig = _lib.call
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(dm, "_RESNET_CONV", mode)
        mp.setattr(dm, "_SHORTCUT_FORK", shortcut_fork)
        mp.setattr(c2, "FORK", fork)
        mp.setattr(c2, "CONV_EXT", front == "ext")
        mp.setattr(c2, "WGRAD_GROUPED", True)
        mp.setattr(bn2d, "FUSED_BN2D", True)
        if front == "python":   # the BatchNorm Functions of bn2d.py as well, so that their entry points are seen below
            mp.setattr(_lib, "torch_ext", lambda: None)
        torch.manual_seed(0)
        stage = getattr(dm.ResNet50(), "layer%d" % k)[:2]
        stage.load_state_dict(rt.canonical_state(name, norm_eval), strict=True)
        stage = stage.to(dev).to(memory_format=torch.channels_last)
        rt.set_norm_eval(stage) if norm_eval else stage.train()
        cache = c2.TransposedWeights(stage.modules()) if cached else None
        mp.setattr(_lib, "call", lambda fn, *a: (calls.append(fn), orig(fn, *a))[1])
        xs, seeds = rt.make_inputs(k, n, h, w)
        res = rt.train_steps(stage, xs, seeds, device=dev, autocast=None if fp32 else torch.bfloat16, channels_last=True,
                             input_dtype=torch.float32 if fp32 else torch.bfloat16)
        torch.cuda.synchronize()
    info = dict(calls=collections.Counter(c for c in calls if c in CONV_AND_BN),
                pending=ext.pending_wgrads() if front == "ext" else 0,
                cached=len(cache.items) if cache is not None else 0)
    assert not c2._PENDING
    _RUNS[key] = (res, info)
    return _RUNS[key]


def _check_parity(res, name, lib_fwd, title, norm_eval=False):
    ref, floors = rt.reference(name, lib_fwd, norm_eval)
    measured = rt.measure(res, ref)
    print(rt.report(measured, floors, title))
    print("GPU " + rt.table_row(name, rt.summary(measured)) + "   # " + title)
    assert rt.batches_tracked(res) == rt.batches_tracked(ref)
    assert set(rt.batches_tracked(res).values()) == ({0} if norm_eval else {STEPS})
    over = rt.violations(measured, floors)
    assert not over, (title, [(n, "%.3g > %.3g" % (v, b)) for n, v, b in over[:8]], len(over))
    # the project's bf16 criteria (tests/test_dense_modules_gpu.py) never relax
    for i in range(STEPS):
        assert measured["out%d.l2" % i] <= 1e-2 * N_CONVS ** 0.5
        for n_, v in measured.items():
            if n_.startswith(("gin%d." % i, "g%d." % i)) and n_.endswith((".l2", ".ang")):
                assert v <= 0.2, (title, n_, v)     # .ang <= 0.2 is cos >= 0.98
    return measured


CASE_MODE = [(name, mode) for name in rt.CASES for mode in ("tuned", "hip")]


@pytest.mark.parametrize("front", ["python", "ext"])
@pytest.mark.parametrize("cached", [True, False], ids=["fused_addend", "torch_add"])
@pytest.mark.parametrize("name,mode", CASE_MODE)
def test_stage_takes_the_hip_path_and_matches_the_rounding_twin(dev, name, mode, cached, front):
    res, info = _run(dev, name, mode, cached, front)
    want = _expected_calls(name, mode, cached, True)
    print("%s %s calls: %s" % (name, mode, dict(sorted(info["calls"].items()))))
    if front == "python":
        assert info["calls"] == want, (sorted(info["calls"].items()), sorted(want.items()))
    else:
        assert not info["calls"] and info["pending"] == 0       # nothing went through ctypes, no weight gradient left queued
    if cached:   # every layer with a HIP data gradient found its transposed weight
        assert info["cached"] == sum(1 for r in _layers(name, mode, True) if r[10])
    _check_parity(res, name, _lib_fwd(name, mode, True), "%s %s %s %s" % (name, mode, "cached" if cached else "uncached", front))


@pytest.mark.parametrize("switch", ["FORK", "_SHORTCUT_FORK"])
@pytest.mark.parametrize("name", list(rt.CASES))
def test_plain_path_without_the_forks_is_the_same_function(dev, name, switch):
    """conv2d.FORK = False / dense_modules._SHORTCUT_FORK = False: autograd adds the skip gradient and the stride-2 shortcut runs
    as a library layer on the full-size input -- same twin (the shortcut's BatchNorm now reads the bf16 tensor), same rule."""
    fork, shortcut = switch != "FORK", switch != "_SHORTCUT_FORK"
    forked = fork and shortcut
    res, info = _run(dev, name, "tuned", True, "python", fork=fork, shortcut_fork=shortcut)
    want = _expected_calls(name, "tuned", True, forked)
    assert info["calls"] == want, (sorted(info["calls"].items()), sorted(want.items()))
    _check_parity(res, name, _lib_fwd(name, "tuned", forked), "%s tuned %s=False" % (name, switch))


@pytest.mark.parametrize("cached", [True, False], ids=["fused_addend", "torch_add"])
@pytest.mark.parametrize("name,mode", CASE_MODE)
def test_front_ends_agree(dev, name, mode, cached):
    """conv2d.py / bn2d.py's Python Functions and csrc/torch_binding.cpp launch the same kernels with the same arguments: outputs, input
    gradient and running statistics are bit-identical and the weight gradients (grouped launch) agree within 2^-7 wherever no library
    convolution is involved: "hip", and "tuned" up to layer3.

    layer4 "tuned" is the exception, and the launch that differs is named: the LIBRARY forward of the 512-channel 3x3 convolutions
    (`0.conv2`, then `1.conv2`).  Forward hooks on every layer show `0.bn1` and `0.downsample.1` bit-identical and `0.conv2` as the
    first tensor that differs (relative L2 2-3e-5) -- between the front-ends, between two runs of the SAME front-end, and between
    three calls of F.conv2d on the same operands in one process: the library's kernel is not deterministic run to run.  Those few
    flipped bf16 roundings grow through the BN + ReLU stack to the reference's own noise level (2.4e-3 at the output, 3e-2 on the
    gradients), so no fixed tolerance below it can hold there; the two runs are instead held to the acceptance rule of the twin
    (margin x floor, each run against the other), i.e. they may differ by no more than an accumulation order explains."""
    py, ex = _run(dev, name, mode, cached, "python")[0], _run(dev, name, mode, cached, "ext")[0]
    exact = mode == "hip" or rt.CASES[name][0] <= 3
    for i in range(STEPS):
        for what in ("out", "gin"):
            print("%s %s %s%d: rel l2 %.3e" % (name, mode, what, i, rt.rel_l2(py[what][i], ex[what][i])))
    if not exact:
        _, floors = rt.reference(name, _lib_fwd(name, mode, True))
        measured = rt.measure(py, ex)
        print(rt.report(measured, floors, "%s %s python against ext" % (name, mode)))
        assert not rt.violations(measured, floors), rt.violations(measured, floors)[:8]
        return
    for i in range(STEPS):
        for what in ("out", "gin"):
            assert torch.equal(py[what][i], ex[what][i]), (what, i)
        for n_, g in ex["grads"][i].items():
            assert rt.rel_l2(py["grads"][i][n_], g) <= 2.0 ** -7, (n_, rt.rel_l2(py["grads"][i][n_], g))
    for n_, b in ex["buffers"].items():
        assert torch.equal(py["buffers"][n_], b), n_


@pytest.mark.parametrize("front", ["python", "ext"])
@pytest.mark.parametrize("mode", ["tuned", "hip"])
def test_norm_eval_stage_ignores_the_statistics_hand_over(dev, mode, front):
    """mmdet's norm_eval on layer2: the BatchNorms run on (randomised) running statistics while the convolutions train, so every HIP
    forward still emits partial sums that the eval-mode BatchNorm must ignore; running statistics and counters must not move."""
    name = "K2"
    launches = dict(bn2d.EVAL_LAUNCHES)
    fresh = ("K2", mode, True, front, True, True, True, False) not in _RUNS
    res, info = _run(dev, name, mode, True, front, norm_eval=True)
    if fresh:
        assert bn2d.EVAL_LAUNCHES["fwd"] == launches["fwd"] + 7 * STEPS and bn2d.EVAL_LAUNCHES["bwd"] == launches["bwd"] + 7 * STEPS
    if front == "python":
        assert not any(k.startswith("bfhip_bn2d") for k in info["calls"]) and info["calls"]["bfhip_conv2d_fwd"] == N_CONVS * STEPS
    state = rt.canonical_state(name, True)
    for n_, b in res["buffers"].items():
        assert torch.equal(b, state[n_].double()), n_
    _check_parity(res, name, frozenset(), "K2 %s norm_eval %s" % (mode, front), norm_eval=True)


def test_fp32_stage_without_autocast(dev):
    """fp32 throughout: library convolutions and the fused fp32 BatchNorm (with residual) against the plain fp64 twin; 1e-3 max-norm
    forward and buffers, the fp32 gradient criteria of tests/test_dense_modules_gpu.py (relative L2 <= 5e-3, 99 % of the elements
    within 5e-3 of the largest)."""
    name = "K2"
    res, info = _run(dev, name, "tuned", True, "python", fp32=True)
    assert info["calls"]["bfhip_bn2d_fwd"] == 7 * STEPS and info["calls"]["bfhip_bn2d_bwd"] == 7 * STEPS
    assert not any(k.startswith("bfhip_conv2d") and k != "bfhip_conv2d_wgrad_group_launch" and info["calls"][k] for k in info["calls"])
    ref = rt.plain_reference(name, torch.float64)

    def max_norm(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))

    def grad_ok(a, b):
        inside = float(((a - b).abs() <= 5e-3 * b.abs().max()).float().mean()) if b.numel() >= 1000 else 1.0
        return inside >= 0.99 and rt.rel_l2(a, b) <= 5e-3, (inside, rt.rel_l2(a, b))

    assert set(rt.batches_tracked(res).values()) == {STEPS}
    for i in range(STEPS):
        print("out%d max-norm %.3e  gin%d %s" % (i, max_norm(res["out"][i], ref["out"][i]), i, grad_ok(res["gin"][i], ref["gin"][i])[1]))
        assert max_norm(res["out"][i], ref["out"][i]) <= 1e-3
        ok, val = grad_ok(res["gin"][i], ref["gin"][i])
        assert ok, ("input grad", i, val)
        for n_, g in ref["grads"][i].items():
            ok, val = grad_ok(res["grads"][i][n_], g)
            assert ok, (n_, i, val)
    m = rt.measure(res, ref, profiles=False)
    for n_, v in m.items():
        if n_.startswith(("rm.", "rv.")):
            assert v <= 1e-3, (n_, v)
