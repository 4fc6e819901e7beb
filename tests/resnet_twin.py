"""A plain torch.nn twin of one ResNet-50 stage prefix (`layerK[:2]`: the projection / down-sampling bottleneck followed by one
identity bottleneck), the metrics the stage tests compare with, and a table of deliberately wrong twins (helper module: no tests).

Nothing here imports the product: the twin is the standard ResNet-50 bottleneck (He et al. 2015, v1.5: the stride sits on the 3x3
convolution) written with nn.Conv2d, nn.BatchNorm2d, F.relu and an explicit `out + identity`, with the usual child names
(`conv1 bn1 conv2 bn2 conv3 bn3 downsample.0 downsample.1`), so `stage(k).load_state_dict(ResNet50().layerK[:2].state_dict(),
strict=True)` pins the state-dict layout as well.

Two ways to evaluate it
-----------------------
rounding=False   the plain graph in the module's dtype (fp32: what the product must equal on the CPU; fp64: the reference of
                 the fp32 GPU case).
rounding=True    the same graph in the module's dtype (fp64 = the reference, fp32 = the reference's own noise) with a
                 straight-through bf16 rounding function `bf16_ste` at the tensor boundaries where the product under bf16 autocast
                 materialises a bf16 tensor.  `bf16_ste` rounds its argument to bf16 in the forward and rounds the incoming
                 gradient to bf16 in the backward (`grad=False`: forward only).  The rounding points, with the product line
                 each mirrors (paths below bevfusion_amd/):
  R1  weights, forward only          conv2d.py `_weight_ohwi` / `TransposedWeights` (bf16 copies of the fp32 parameter; the
                                     weight gradient is written in the parameter's dtype: `_launch_wgrad`, `_flush_wgrads`)
  R2  every convolution output       conv2d.py `_Conv2dFunction.forward`: `y = torch.empty(..., dtype=torch.bfloat16)`; backward:
                                     its incoming gradient is the BatchNorm's `dx = torch.empty_like(x)` (bn2d.py
                                     `_BN2dFunction.backward`), bf16
  R3  BN (+ ReLU) output             bn2d.py `_BN2dFunction.forward`: `y = torch.empty_like(x)`; backward: the incoming gradient is
                                     the next convolution's `dx` (conv2d.py `_hip_dgrad`: `dx = torch.empty(..., bfloat16)`)
  R4  BN + residual + ReLU output    the same `y`, rounded ONCE after the add (csrc/bn2d.hip applies scale, shift, residual and
                                     ReLU in fp32 registers); backward: the gradient that reaches a block's output is the sum of
                                     the next block's conv1 data gradient and its skip gradient, rounded once where the add is
                                     fused into the data gradient's epilogue (conv2d.py `_hip_dgrad(..., addend)`)
  R5  the stage input, backward only the input gradient is the same fused sum, a bf16 tensor
  R6  the shortcut's input, backward the compact data gradient of the stride-2 shortcut is a bf16 tensor before it is added at the
      only                           even pixels (conv2d.py `_hip_dgrad` called from `forward_unstrided`'s node)
  S   BatchNorm batch statistics     a HIP forward hands the BatchNorm the column sums of its fp32 ACCUMULATORS
                                     (`y._bfhip_stat_partial`, conv2d.py `Conv2dHipWgrad.forward`), so mean and variance are those of
                                     the unrounded convolution output while the normalised tensor is the rounded one; behind a
                                     library forward (the names in `lib_fwd`) bn2d.py's own statistics pass reads the bf16 tensor.
                                     Found on paper before the first GPU run: with statistics of the rounded tensor the floors
                                     of the running means would have been those of a handful of flipped roundings (1e-7) against
                                     an expected 2^-9 |y| / sqrt(pixels) ~ 4e-5 standard deviations on the GPU.
The parameters of the BatchNorms stay fp32 and unrounded, as in the product.  fp64 -> bf16 goes through fp32 (torch's
conversion); the double rounding matters only at exact ties of the fp32 value.

Metrics (`measure`)
-------------------
For every step: outputs and input gradient -- relative L2 `l2`, angle `ang` = sqrt(2 (1 - cos)) (it scales like l2, so one margin
serves both; cos >= 0.98 is ang <= 0.2) and the PROFILE maxima `row`, `col`, `img`, `ch8`: the largest relative L2 over every image
row, every image column, every batch image and every block of 8 channels (a wrong edge row / column, batch stride or channel block
moves one of them by a factor while the global figure hardly moves).  Every parameter gradient: `l2`, `ang`.  After the last step:
`rm` = max |running mean difference| / running standard deviation, `rv` = max |running variance difference| / max running
variance, per BatchNorm; `num_batches_tracked` is read through state_dict() and compared exactly.

Acceptance rule (`violations`): every metric <= margin x its floor, margin 3 for global metrics, 2.5 for profile maxima; the floor
of a metric is its value between this twin (rounding=True) run in fp32 and run in fp64 -- the reference's own sensitivity to the
accumulation order, no product involved.  The floors of the running
statistics (`rm`, `rv`) of the first layers are those of a handful of flipped roundings (1e-7 .. 1e-10): below what ANY fp32
statistics pass can reach, so they are lifted to FLOOR_STAT = 2 * 2^-24 * sqrt(2048) ~ 5.4e-6 -- two fp32 sums (sum, sum of squares)
of >= 2048 terms in an arbitrary order, rounding errors adding like a random walk.  (Mutant d sits at 0.19 / 2161 ~ 9e-5.)

Floors (CPU, fp32 against fp64 rounding twin, two steps, worst step; tests/test_resnet_twin_cpu.py prints and re-checks them)
-----------------------------------------------------------------------------------------------------------------------------
case       out.l2  out.row  out.col  out.img  out.ch8   gin.l2  gin.row  gin.col  gin.img  gin.ch8    gw.l2   gbn.l2       rm       rv
K1       1.6e-03  1.9e-03  2.1e-03  1.6e-03  1.8e-03  2.2e-02  3.3e-02  5.1e-02  2.4e-02  2.2e-02  2.5e-02  2.6e-02  5.1e-06  4.2e-06
K2       3.0e-03  3.2e-03  3.3e-03  3.0e-03  3.5e-03  3.9e-02  4.8e-02  5.7e-02  4.0e-02  4.0e-02  4.3e-02  4.9e-02  7.4e-06  8.6e-06
K2even   2.8e-03  3.0e-03  3.3e-03  2.8e-03  3.2e-03  4.2e-02  5.1e-02  5.6e-02  4.3e-02  4.2e-02  4.6e-02  5.8e-02  7.7e-06  6.8e-06
K3       3.0e-03  3.2e-03  3.3e-03  3.0e-03  3.6e-03  4.4e-02  5.2e-02  5.7e-02  4.5e-02  4.5e-02  5.0e-02  5.8e-02  1.0e-05  1.0e-05
K4       3.3e-03  3.4e-03  3.6e-03  3.3e-03  3.8e-03  4.8e-02  5.5e-02  5.8e-02  4.9e-02  4.8e-02  5.3e-02  6.5e-02  1.3e-05  1.2e-05
(cases: tests/resnet_twin.py `CASES`; out / gin = stage output / input gradient; gw / gbn = the worst convolution-weight /
BatchNorm-parameter gradient; the tests use the per-metric, per-parameter floors computed the same way, of which these are the
worst per family)

Mutants (`MUTANTS`): one deliberate mistake each, of the kind the hand-wired trunk could make; every one must be rejected by the
acceptance rule with a factor >= 2 to spare (tests/test_resnet_twin_cpu.py).
"""
import contextlib
import math

import torch
import torch.nn.functional as F
from torch import nn

#       K: (inplanes, planes, stride) of layerK's first block (torchvision / mmdet ResNet-50)
STAGES = {1: (64, 64, 1), 2: (256, 128, 2), 3: (512, 256, 2), 4: (1024, 512, 2)}

MUTANTS = {
    "a": "skip gradient dropped on the last row and the last column of the map",
    "b": "stride-2 shortcut reads (and scatters its gradient at) the odd pixels",
    "c": "residual added after the ReLU",
    "d": "running variance updated with the biased batch variance",
    "e": "bn3's ReLU backward mask taken from BN(x) > 0 instead of BN(x) + identity > 0",
    "f": "shortcut BatchNorm normalised with conv3's batch statistics",
}

MARGIN_GLOBAL, MARGIN_PROFILE = 3.0, 2.5
PROFILE_KEYS = ("row", "col", "img", "ch8")
FLOOR_STAT = 2.0 * 2.0 ** -24 * math.sqrt(2048.0)


class _Bf16Ste(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, fwd, grad):
        ctx.grad = grad
        return t.to(torch.bfloat16).to(t.dtype) if fwd else t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return (g.to(torch.bfloat16).to(g.dtype) if ctx.grad else g), None, None


def bf16_ste(t, fwd=True, grad=True):
    """t rounded to bf16 (kept in t's dtype); straight-through, the incoming gradient rounded to bf16 as well (`grad`)."""
    return _Bf16Ste.apply(t, fwd, grad)


class _DropEdgeGrad(torch.autograd.Function):
    """Identity whose gradient loses its last row and last column (mutant a)."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[:, :, -1, :] = 0
        g[:, :, :, -1] = 0
        return g


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, rounding=False, mutant=None, lib_fwd=(), prefix=""):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample
        self.rounding, self.mutant, self.lib_fwd, self.prefix = rounding, mutant, frozenset(lib_fwd), prefix

    # ---- pieces
    def _conv(self, name, conv, x):
        """(the tensor the next layer reads, the tensor the BatchNorm behind it takes its statistics from)"""
        if not self.rounding:
            y = conv(x)
            return y, y
        acc = F.conv2d(x, bf16_ste(conv.weight, grad=False), None, conv.stride, conv.padding)        # R1
        y = bf16_ste(acc)                                                                              # R2
        if self.prefix + name in self.lib_fwd:
            return y, y                                       # S: statistics pass over the bf16 tensor
        return y, y + (acc - y).detach()                      # S: the value of the accumulators, the gradient path of y

    def _bn(self, bn, x, src):
        old_var = bn.running_var.clone() if (self.mutant == "d" and bn.training) else None
        if not bn.training or (src is x and not self.rounding):
            y = bn(x)
        else:
            y = batch_norm_train(bn, x, src)
        if old_var is not None:
            with torch.no_grad():
                bn.running_var.copy_((1 - bn.momentum) * old_var + bn.momentum * src.var((0, 2, 3), unbiased=False))
        return y

    def _act(self, t, relu=True):
        t = F.relu(t) if relu else t
        return bf16_ste(t) if self.rounding else t            # R3 / R4

    def _shortcut(self, x, src3):
        conv, bn = self.downsample[0], self.downsample[1]
        if self.rounding:
            x = bf16_ste(x, fwd=False)                         # R6
        if self.mutant == "b" and conv.stride == (2, 2):
            x = F.pad(x, (0, 1, 0, 1))[:, :, 1:, 1:]           # the odd pixels (zero past the edge)
        y, src = self._conv("downsample.0", conv, x)
        if self.mutant == "f" and bn.training:
            return self._act(batch_norm_train(bn, y, src3.detach()), relu=False)
        return self._act(self._bn(bn, y, src), relu=False)

    def forward(self, x):
        skip = _DropEdgeGrad.apply(x) if self.mutant == "a" else x
        out, src = self._conv("conv1", self.conv1, x)
        out = self._act(self._bn(self.bn1, out, src))
        out, src = self._conv("conv2", self.conv2, out)
        out = self._act(self._bn(self.bn2, out, src))
        out, src = self._conv("conv3", self.conv3, out)
        identity = skip if self.downsample is None else self._shortcut(skip, src)
        out = self._bn(self.bn3, out, src)
        if self.mutant == "c":
            return self._act(F.relu(out) + identity, relu=False)
        if self.mutant == "e":
            z = out + identity
            keep = (out > 0).to(z.dtype).detach()
            return self._act(z * keep + (F.relu(z) - z * keep).detach(), relu=False)    # value relu(z), gradient through `keep`
        return self._act(out + identity)


def batch_norm_train(bn, x, src):
    """Training-mode BatchNorm of x with the batch statistics of `src` (same shape): the textbook formulas, running statistics
    updated like nn.BatchNorm2d (momentum, unbiased variance, num_batches_tracked)."""
    n = src.numel() // src.shape[1]
    mean = src.mean((0, 2, 3))
    var = src.var((0, 2, 3), unbiased=False)
    with torch.no_grad():
        bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean.detach())
        bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * var.detach() * (n / (n - 1)))
        bn.num_batches_tracked += 1
    scale = bn.weight * torch.rsqrt(var + bn.eps)
    return (x - mean[None, :, None, None]) * scale[None, :, None, None] + bn.bias[None, :, None, None]


class Stage(nn.Sequential):
    """layerK[:2]; in rounding mode the input's gradient is a bf16 tensor (R5)."""

    rounding = False

    def forward(self, x):
        if self.rounding:
            x = bf16_ste(x, fwd=False)
        return super().forward(x)


def stage(k, rounding=False, mutant=None, lib_fwd=()):
    inplanes, planes, stride = STAGES[k]
    down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
    s = Stage(Bottleneck(inplanes, planes, stride, down, rounding, mutant, lib_fwd, "0."),
              Bottleneck(planes * 4, planes, 1, None, rounding, mutant, lib_fwd, "1."))
    s.rounding = rounding
    return s


# ---------------------------------------------------------------------------------------------------------------- running it
def bf16_tensor(shape, seed, scale=1.0):
    """A bf16-representable fp32 tensor of standard normals times `scale`."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).float()


def out_hw(k, h, w):
    s = STAGES[k][2]
    return (h - 1) // s + 1, (w - 1) // s + 1


def make_inputs(k, n, h, w, steps=2, seed=0):
    """(inputs, loss seeds) of `steps` training steps: bf16-representable, a different pair every step."""
    inplanes, planes, _ = STAGES[k]
    oh, ow = out_hw(k, h, w)
    xs = [bf16_tensor((n, inplanes, h, w), 1000 * k + 10 * seed + i) for i in range(steps)]
    # (post-ReLU stage inputs are non-negative in the network; the sign does not matter to any kernel)
    seeds = [bf16_tensor((n, planes * 4, oh, ow), 2000 * k + 10 * seed + i, 1.0 / math.sqrt(n * planes * 4 * oh * ow))
             for i in range(steps)]
    return xs, seeds


def randomise(module, seed, running=False):
    """Non-trivial BatchNorm affine parameters (and, for eval-mode BatchNorms, running statistics)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.empty(m.num_features).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.empty(m.num_features).uniform_(-0.3, 0.3, generator=g))
                if running:
                    m.running_mean.copy_(torch.empty(m.num_features).uniform_(-0.2, 0.2, generator=g))
                    m.running_var.copy_(torch.empty(m.num_features).uniform_(0.5, 1.5, generator=g))


def train_steps(module, xs, seeds, device="cpu", autocast=None, channels_last=False, input_dtype=None):
    """One forward + backward per (input, seed) pair on `module` as it stands (its train / eval flags are the caller's); loss =
    sum(out * seed).  Returns fp64 CPU tensors: dict(out=[..], gin=[..], grads=[{name: g}..], buffers={name: b})."""
    dtype = next(module.parameters()).dtype
    res = dict(out=[], gin=[], grads=[])
    for x, s in zip(xs, seeds):
        for p in module.parameters():
            p.grad = None
        x = x.to(device=device, dtype=input_dtype or dtype)
        if channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        x = x.detach().requires_grad_(True)
        ctx = torch.autocast(torch.device(device).type, dtype=autocast) if autocast is not None else contextlib.nullcontext()
        with ctx:
            out = module(x)
        wide = out if out.dtype == torch.float64 else out.float()
        (wide * s.to(device=device, dtype=wide.dtype)).sum().backward()
        res["out"].append(out.detach().double().cpu())
        res["gin"].append(x.grad.detach().double().cpu())
        res["grads"].append({n: p.grad.detach().double().cpu() for n, p in module.named_parameters()})
    res["buffers"] = {n: b.detach().double().cpu() for n, b in module.state_dict().items() if "." in n and n.split(".")[-1] in
                      ("running_mean", "running_var", "num_batches_tracked")}
    return res


# ---------------------------------------------------------------------------------------------------------------- metrics
def rel_l2(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def cosine(a, b):
    return float((a * b).sum() / (a.norm() * b.norm()).clamp_min(1e-300))


def angle(a, b):
    """sqrt(2 (1 - cos)): the relative L2 of the normalised tensors; ~ rel_l2 for small errors."""
    an, bn = a / a.norm().clamp_min(1e-300), b / b.norm().clamp_min(1e-300)
    return float((an - bn).norm())


def profile(a, b):
    """Largest relative L2 over the rows, the columns, the batch images and the blocks of 8 channels of [N, C, H, W] tensors."""
    n, c, h, w = b.shape
    d2, b2 = (a - b).square(), b.square()

    def worst(dims):
        return float((d2.sum(dims).sqrt() / b2.sum(dims).sqrt().clamp_min(1e-300)).max())

    c8 = (c // 8) * 8
    ch = (d2[:, :c8].reshape(n, c8 // 8, 8, h, w).sum((0, 2, 3, 4)).sqrt()
          / b2[:, :c8].reshape(n, c8 // 8, 8, h, w).sum((0, 2, 3, 4)).sqrt().clamp_min(1e-300))
    return dict(row=worst((0, 1, 3)), col=worst((0, 1, 2)), img=worst((1, 2, 3)), ch8=float(ch.max()))


def measure(got, want, profiles=True):
    """name -> value of every metric of the module docstring between two `train_steps` results (the second is the reference)."""
    m = {}
    for i in range(len(want["out"])):
        for what in ("out", "gin"):
            a, b = got[what][i], want[what][i]
            assert a.shape == b.shape, (what, a.shape, b.shape)
            key = "%s%d" % (what, i)
            m[key + ".l2"], m[key + ".ang"] = rel_l2(a, b), angle(a, b)
            if profiles:
                for k, v in profile(a, b).items():
                    m["%s.%s" % (key, k)] = v
        assert set(got["grads"][i]) == set(want["grads"][i])
        for n, b in want["grads"][i].items():
            a = got["grads"][i][n]
            m["g%d.%s.l2" % (i, n)], m["g%d.%s.ang" % (i, n)] = rel_l2(a, b), angle(a, b)
    for n, b in want["buffers"].items():
        if n.endswith("running_mean"):
            sd = want["buffers"][n.replace("running_mean", "running_var")].sqrt()
            m["rm." + n[:-len(".running_mean")]] = float(((got["buffers"][n] - b).abs() / sd).max())
        elif n.endswith("running_var"):
            m["rv." + n[:-len(".running_var")]] = float((got["buffers"][n] - b).abs().max() / b.abs().max())
    return m


def batches_tracked(res):
    return {n: int(b) for n, b in res["buffers"].items() if n.endswith("num_batches_tracked")}


def margin(name):
    return MARGIN_PROFILE if name.rsplit(".", 1)[-1] in PROFILE_KEYS else MARGIN_GLOBAL


def bound(name, floors):
    floor = floors[name]
    if name.startswith(("rm.", "rv.")):
        floor = max(floor, FLOOR_STAT)
    return margin(name) * floor


def violations(measured, floors):
    """[(metric, value, bound)] of every metric over margin x floor (the acceptance rule)."""
    return [(n, v, bound(n, floors)) for n, v in sorted(measured.items()) if not v <= bound(n, floors)]


def report(measured, floors, title):
    """The printed record: every measured value next to its bound."""
    lines = [title]
    for n, v in sorted(measured.items()):
        lines.append("  %-44s %.3e  bound %.3e  (floor %.3e)%s" % (n, v, bound(n, floors), floors[n],
                                                                   "" if v <= bound(n, floors) else "   <-- OVER"))
    return "\n".join(lines)


def summary(m):
    """The few figures of a `measure` result that go into the tables: worst step / worst parameter per family."""
    def worst(pred):
        vals = [v for n, v in m.items() if pred(n)]
        return max(vals) if vals else float("nan")
    s = {}
    for what in ("out", "gin"):
        for k in ("l2",) + PROFILE_KEYS:
            s["%s.%s" % (what, k)] = worst(lambda n: n.startswith(what) and n.endswith("." + k))
    s["gw.l2"] = worst(lambda n: n.startswith("g") and n.endswith(".weight.l2") and ("conv" in n or "downsample.0" in n))
    s["gbn.l2"] = worst(lambda n: n[0] == "g" and n[1].isdigit() and n.endswith(".l2") and ("bn" in n or "downsample.1" in n))
    s["rm"] = worst(lambda n: n.startswith("rm."))
    s["rv"] = worst(lambda n: n.startswith("rv."))
    return s


# ---------------------------------------------------------------------------------------------------------------- shared cases
#        name: (K, N, H, W).  Output maps 23 x 47 (odd: the last row / column is an even pixel and every tile is partial) with
#        2 * 23 * 47 = 2162 >= 2048 pixels, the smallest the HIP convolutions take; one even-sized case: 44 x 96 -> 22 x 48 = 2112
#        pixels (44 x 92 -> 22 x 46 is 2024 pixels, under the 2048 below which the second block would go to the library)
CASES = {"K1": (1, 2, 23, 47), "K2": (2, 2, 45, 93), "K2even": (2, 2, 44, 96), "K3": (3, 2, 45, 93), "K4": (4, 2, 45, 93)}
_MEMO = {}


def canonical_state(name, norm_eval=False):
    """The state every run of a case starts from: torch's default initialisation, non-trivial BatchNorm affine parameters; random
    running statistics for eval-mode BatchNorms (`norm_eval`), the default ones (0, 1) otherwise."""
    key = ("state", name)
    if key not in _MEMO:
        k = CASES[name][0]
        torch.manual_seed(100 + k)
        s = stage(k)
        randomise(s, 7 + k, running=True)
        _MEMO[key] = {n: v.clone() for n, v in s.state_dict().items()}
    state = {n: v.clone() for n, v in _MEMO[key].items()}
    if not norm_eval:
        for n, v in state.items():
            if n.endswith("running_mean"):
                v.zero_()
            elif n.endswith("running_var"):
                v.fill_(1.0)
    return state


def set_norm_eval(module):
    """mmdet's norm_eval: every BatchNorm on its running statistics, the convolutions in training mode."""
    module.train()
    for m in module.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.eval()
    return module


def twin_run(name, dtype, rounding=True, mutant=None, lib_fwd=(), norm_eval=False):
    k, n, h, w = CASES[name]
    s = stage(k, rounding=rounding, mutant=mutant, lib_fwd=lib_fwd)
    s.load_state_dict(canonical_state(name, norm_eval), strict=True)
    s.to(dtype)
    set_norm_eval(s) if norm_eval else s.train()
    return train_steps(s, *make_inputs(k, n, h, w))


def reference(name, lib_fwd=(), norm_eval=False):
    """(fp64 rounding twin, floors) of a case, computed once per process and never modified."""
    key = ("ref", name, tuple(sorted(lib_fwd)), norm_eval)
    if key not in _MEMO:
        ref = twin_run(name, torch.float64, True, None, lib_fwd, norm_eval)
        _MEMO[key] = (ref, measure(twin_run(name, torch.float32, True, None, lib_fwd, norm_eval), ref))
    return _MEMO[key]


def plain_reference(name, dtype=torch.float32, norm_eval=False):
    """The plain twin (no rounding model) on the CPU."""
    key = ("plain", name, dtype, norm_eval)
    if key not in _MEMO:
        _MEMO[key] = twin_run(name, dtype, False, None, (), norm_eval)
    return _MEMO[key]


SUMMARY_COLUMNS = ("out.l2", "out.row", "out.col", "out.img", "out.ch8", "gin.l2", "gin.row", "gin.col", "gin.img", "gin.ch8",
                   "gw.l2", "gbn.l2", "rm", "rv")


def table_row(name, s):
    return "%-7s" % name + "".join(" %8.1e" % s[c] for c in SUMMARY_COLUMNS)


def floor_table():
    """The floors table of the module docstring: case -> {column: value}."""
    rows = {}
    for line in __doc__.splitlines():
        parts = line.split()
        if parts and parts[0] in CASES and len(parts) == 1 + len(SUMMARY_COLUMNS):
            rows[parts[0]] = dict(zip(SUMMARY_COLUMNS, map(float, parts[1:])))
    return rows
