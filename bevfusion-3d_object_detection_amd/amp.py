"""bf16 parameters with fp32 master weights for the dense (MFMA) layers.

Under plain autocast every conv / linear weight is re-cast fp32 -> bf16 in each forward and its bf16 gradient is cast
back to fp32 in each backward: ~320 tiny launches per step for this model.  Here the weights of those layers ARE bf16
(what the kernels consume), the optimizer owns fp32 master copies, and the two conversions are one multi-tensor copy
each per step.  The arithmetic is unchanged: the forward uses the same bf16 values autocast would produce and the weight
gradient the same bf16 tensor the bf16 kernels emit.  With DDP the gradient all-reduce of these layers moves half the
bytes (bf16 buckets).  Layers that the model runs in fp32 islands, BatchNorm / LayerNorm and the sparse encoder keep
fp32 parameters."""
import os

import torch
from torch import nn

_LOW_TYPES = (nn.Conv1d, nn.Conv2d, nn.ConvTranspose2d, nn.Linear, nn.MultiheadAttention)


def low_precision_parameters(model, exclude=("pts_middle_encoder", "heatmap_head")):
    """Parameters of the conv / linear / attention-projection layers that run under bf16 autocast."""
    out, seen = [], set()
    for name, mod in model.named_modules():
        if any(part in name.split(".") for part in exclude) or not isinstance(mod, _LOW_TYPES):
            continue
        for p in mod.parameters(recurse=False):
            if p.requires_grad and p.dtype == torch.float32 and id(p) not in seen:
                seen.add(id(p))
                out.append(p)
    return out


def skip_nonfinite_step(opt, total_norm):
    """A step whose gradient norm is NaN / inf leaves parameters, moments and step counters untouched -- decided on the
    device (the fused AdamW kernels' `found_inf` input, what GradScaler uses), no host read.  This is how a poisoned loss
    (an invalid Hungarian cost matrix; a frame that overflowed a static row capacity, BEVFusion.loss) costs one skipped
    step instead of NaN weights.  The reference's OptimWrapper has no such guard: with it a NaN loss ends the run."""
    opt.found_inf = (~torch.isfinite(total_norm)).to(torch.float32).reshape(())
    opt.grad_scale = None


_NORM_TYPES = (nn.modules.batchnorm._BatchNorm, nn.modules.instancenorm._InstanceNorm, nn.LayerNorm, nn.GroupNorm)
_PARAMWISE_KEYS = ("custom_keys", "norm_decay_mult", "bias_decay_mult")


def build_param_groups(model, lr, weight_decay, paramwise_cfg=None):
    """Parameter groups of `model`'s trainable parameters: a list of (dict(lr=, weight_decay=), [parameter names]).

    `paramwise_cfg` follows the subset of mmengine's DefaultOptimWrapperConstructor that BEVFusion recipes use (from knowledge
    of that package, parity unpinned: mmengine is not among this project's dependencies):
      custom_keys      {substring of the parameter name: dict(lr_mult=1.0, decay_mult=1.0)}; of the keys that occur in a name the
                       longest wins, ties break alphabetically; a match overrides the two rules below
      norm_decay_mult  weight-decay multiplier of the parameters (weight and bias) of _BatchNorm / _InstanceNorm / LayerNorm /
                       GroupNorm modules, which includes this package's fused norm modules (subclasses of torch's)
      bias_decay_mult  weight-decay multiplier of parameters named `bias` of every other module
    Parameters with equal (lr, weight_decay) share a group; groups and the names inside them come in the order of
    `model.named_parameters()` (a group stands where its first parameter does), so the result does not depend on dict order.
    Pure Python over module types and names: no device needed."""
    cfg = dict(paramwise_cfg or {})
    unknown = sorted(set(cfg) - set(_PARAMWISE_KEYS))
    if unknown:
        raise ValueError("paramwise_cfg: unsupported keys %s (supported: %s)" % (unknown, list(_PARAMWISE_KEYS)))
    custom = cfg.get("custom_keys") or {}
    for key, mult in custom.items():
        bad = sorted(set(mult) - {"lr_mult", "decay_mult"})
        if bad:
            raise ValueError("paramwise_cfg: custom_keys[%r]: unsupported entries %s" % (key, bad))
    keys = sorted(sorted(custom), key=len, reverse=True)
    norm_mult, bias_mult = cfg.get("norm_decay_mult"), cfg.get("bias_decay_mult")
    groups, seen = {}, set()
    for mod_name, mod in model.named_modules():
        is_norm = isinstance(mod, _NORM_TYPES)
        for short, p in mod.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            name = mod_name + "." + short if mod_name else short
            g_lr, g_wd = float(lr), float(weight_decay)
            key = next((k for k in keys if k in name), None)
            if key is not None:
                g_lr *= float(custom[key].get("lr_mult", 1.0))
                g_wd *= float(custom[key].get("decay_mult", 1.0))
            elif is_norm:
                if norm_mult is not None:
                    g_wd *= float(norm_mult)
            elif short == "bias" and bias_mult is not None:
                g_wd *= float(bias_mult)
            groups.setdefault((g_lr, g_wd), []).append(name)
    return [(dict(lr=k[0], weight_decay=k[1]), names) for k, names in groups.items()]


class MasterWeightAdamW:
    """AdamW (fused) over fp32 master copies of `low` (converted to bf16 in place) plus the remaining fp32 parameters.

    Hyper-parameters.  `self.opt` is a torch.optim.AdamW over the masters and the fp32 parameters, built with the groups of
    `build_param_groups(model, lr, weight_decay, paramwise_cfg)`; `self.param_groups` IS `self.opt.param_groups`.  Every step of
    every path reads lr, betas, eps and weight_decay of every group from there, so a learning-rate or momentum schedule is a
    torch scheduler constructed on `mw.opt` (torch.optim.lr_scheduler.LinearLR(mw.opt, ...)), or a loop that assigns
    `mw.param_groups[i]["lr"]` / `["betas"]`; call `scheduler.step()` after `mw.step()`.  A skipped step (non-finite gradient
    norm) does not advance the optimizer's step counter, while a scheduler still advances, as with torch's GradScaler.
    `capturable=True` is as before: the step goes through `self.opt` so that it can sit in a captured hipGraph, and the
    hyper-parameters are those at capture time -- a replay does not see later edits of the groups.

    Checkpoints.  `state_dict()` / `load_state_dict()` carry the moments, the one step counter, the groups and the fp32 masters
    (which hold bits that the model's bf16 weights do not); the layout is the same whichever path wrote it, so a state written
    by one path loads into another.  Save `model.state_dict()` next to it: the fp32 parameters live there."""

    def __init__(self, model, lr, weight_decay, max_grad_norm=None, exclude=("pts_middle_encoder", "heatmap_head"),
                 capturable=False, betas=(0.9, 0.999), eps=1e-8, paramwise_cfg=None):
        self.low = low_precision_parameters(model, exclude)
        low_ids = {id(p) for p in self.low}
        self.other = [p for p in model.parameters() if p.requires_grad and id(p) not in low_ids]
        self.master = [p.detach().clone().float() for p in self.low]
        for p in self.low:
            p.data = p.data.to(torch.bfloat16)
        for m in self.master:
            m.grad = torch.zeros_like(m)
        self.max_grad_norm = max_grad_norm
        # Groups.  Tensor i of `master + other` belongs to group _group_of[i]; inside a group the tensors keep the order of
        # `master + other`, so without a paramwise_cfg self.opt is AdamW(master + other), as it always was.
        params = self.master + self.other
        index_of = {id(p): i for i, p in enumerate(self.low + self.other)}
        named = dict(model.named_parameters())
        self._group_of = [0] * len(params)
        self._group_idx = []                       # per group: indices into master + other
        groups = build_param_groups(model, lr, weight_decay, paramwise_cfg)
        for gi, (_, names) in enumerate(groups):
            self._group_idx.append(sorted(index_of[id(named[n])] for n in names))
            for i in self._group_idx[-1]:
                self._group_of[i] = gi
        assert sorted(i for idx in self._group_idx for i in idx) == list(range(len(params))), "a parameter without a group"
        self._opt_order = [i for idx in self._group_idx for i in idx]   # self.opt's parameter order (what its state_dict indexes)
        # capturable: step counters live on the device, so step() can sit inside a captured hipGraph
        self.opt = torch.optim.AdamW([dict(params=[params[i] for i in idx], **hyper) for idx, (hyper, _) in zip(self._group_idx, groups)],
                                     lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, fused=True, capturable=capturable)
        self.param_groups = self.opt.param_groups
        # Direct path (default): the same fused multi-tensor kernels torch.optim.AdamW(fused=True) and clip_grad_norm_ launch,
        # called on lists prepared ONCE -- the optimizer object re-derives its per-parameter lists, state dicts and device
        # groups in Python on every step (2.8 ms of host time per step for the ~450 tensors of this model, on a step whose host
        # and GPU sides are balanced).  Same arithmetic, same found_inf skip; BFHIP_DIRECT_ADAMW=0 goes through the object.
        # Flat path (default, csrc/optim.hip): clipping + AdamW + the bf16 refresh of ALL tensors in three launches from a
        # device-resident table; per step only the gradient pointers and the groups' hyper-parameters are uploaded, in one
        # copy.  BFHIP_FLAT_ADAMW=0 selects the paths below.
        self.flat = (os.environ.get("BFHIP_FLAT_ADAMW", "1") == "1" and not capturable and max_grad_norm is not None
                     and all(p.is_cuda for p in self.master + self.other))
        if self.flat:
            self._build_flat()
        self.direct = os.environ.get("BFHIP_DIRECT_ADAMW", "1") == "1" and not capturable and not self.flat
        if self.direct:
            self._params = self.master + self.other
            dev = self._params[0].device
            self._exp_avg = [torch.zeros_like(p, memory_format=torch.preserve_format) for p in self._params]
            self._exp_avg_sq = [torch.zeros_like(p, memory_format=torch.preserve_format) for p in self._params]
            self._steps_flat = torch.zeros(len(self._params), dtype=torch.float32, device=dev)
            self._steps = list(self._steps_flat.unbind(0))  # 0-d views: one add_ on the flat tensor advances them all
            # one _fused_adamw_ call per group, on lists prepared once; the hyper-parameters are read from the group at every step
            self._direct_groups = [tuple([lst[i] for i in idx] for lst in (self._params, self._exp_avg, self._exp_avg_sq, self._steps))
                                   for idx in self._group_idx]
        # transposed bf16 copies of the conv weights for the HIP data gradients, all layers in one launch after every update
        # (conv2d.TransposedWeights); built last: the parameters have their final storage now.  BFHIP_WT_CACHE=0: per-call transposes
        self.transposed = None
        if os.environ.get("BFHIP_WT_CACHE", "1") == "1" and all(p.is_cuda for p in self.master + self.other):
            from .conv2d import TransposedWeights
            self.transposed = TransposedWeights(model.modules())

    # ------------------------------------------------------------------ flat path
    def _build_flat(self):
        import numpy as np
        from . import _lib
        lib = _lib.load()
        dev = self.master[0].device if self.master else self.other[0].device
        # (parameter whose .grad is read, fp32 master, bf16 copy or None)
        self._flat_items = [(p, m, p) for p, m in zip(self.low, self.master)] + [(p, p.data, None) for p in self.other]
        for _, m, _ in self._flat_items:
            assert m.dtype == torch.float32
        self._flat_m = [torch.zeros_like(m, memory_format=torch.preserve_format) for _, m, _ in self._flat_items]
        self._flat_v = [torch.zeros_like(m, memory_format=torch.preserve_format) for _, m, _ in self._flat_items]
        seg_dt = np.dtype([("master", "<u8"), ("m", "<u8"), ("v", "<u8"), ("lowp", "<u8"), ("n", "<i8"), ("grad_bf16", "<i4"),
                           ("group", "<i4")])
        assert seg_dt.itemsize == lib.bfhip_adamw_segment_bytes()
        chunk = lib.bfhip_adamw_chunk_elems()
        segs = np.zeros(len(self._flat_items), seg_dt)
        chunks = []
        for i, ((p, m, low), em, ev) in enumerate(zip(self._flat_items, self._flat_m, self._flat_v)):
            # element i of every array of a record must be the same logical element: all share the parameter's dense layout
            assert em.stride() == m.stride() and (low is None or low.stride() == m.stride()), "layout mismatch"
            segs[i] = (m.data_ptr(), em.data_ptr(), ev.data_ptr(), low.data_ptr() if low is not None else 0, m.numel(),
                       1 if low is not None else 0, self._group_of[i])
            chunks += [(i, c) for c in range(-(-m.numel() // chunk))]
        self._n_chunks = len(chunks)
        self._segs_dev = torch.from_numpy(segs.view(np.uint8).copy()).to(dev)
        self._chunks_dev = torch.tensor(chunks, dtype=torch.int32, device=dev)
        self._partial_dev = torch.empty(self._n_chunks, dtype=torch.float32, device=dev)
        self.scalars = torch.zeros(8, dtype=torch.float32, device=dev)  # [0] clip, [1] found_inf, [2] step, [5] gradient norm
        # What changes per step, one image = one H2D copy: int64[n] gradient pointers, then f32[n_groups][8] group records
        # (lr, beta1, beta2, eps, weight_decay written here; the kernels fill in the bias corrections on the device).  Two
        # pinned host images alternate, and an event recorded after each upload is waited for before that image is rewritten: a
        # host that runs ahead of the device by two steps must not overwrite pointers or a learning rate not yet copied.
        n, n_groups = len(self._flat_items), len(self.param_groups)
        self._img_host = [torch.zeros(n + 4 * n_groups, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._img_ptrs = [t.numpy()[:n] for t in self._img_host]
        self._img_groups = [t.numpy()[n:].view(np.float32).reshape(n_groups, 8) for t in self._img_host]
        self._img_groups_addr = [a.ctypes.data for a in self._img_groups]
        self._img_event = [torch.cuda.Event() for _ in range(2)]
        self._img_dev = torch.zeros(n + 4 * n_groups, dtype=torch.int64, device=dev)
        self._groups_dev_addr = self._img_dev.data_ptr() + 8 * n
        self._flip = 0
        self._grad_dtype = [torch.bfloat16 if low is not None else torch.float32 for _, _, low in self._flat_items]

    def _step_flat(self):
        from . import _lib
        ptrs, keep = [], []
        for (p, m, _), dt in zip(self._flat_items, self._grad_dtype):
            g = p.grad
            if g is None:
                ptrs.append(0)
                continue
            if g.dtype != dt or g.stride() != m.stride():
                # a gradient that is not laid out like its parameter (or not in its dtype): one conforming copy
                c = torch.empty_strided(m.size(), m.stride(), dtype=dt, device=m.device)
                c.copy_(g)
                keep.append(c)
                g = c
            ptrs.append(g.data_ptr())
        k = self._flip
        self._flip ^= 1
        self._img_event[k].synchronize()     # the upload that last read this image; normally long complete
        self._img_ptrs[k][:] = ptrs
        rec = self._img_groups[k]
        for i, g in enumerate(self.param_groups):
            rec[i, :5] = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
        self._img_dev.copy_(self._img_host[k], non_blocking=True)
        self._img_event[k].record()
        _lib.call("bfhip_adamw_step_groups", self._segs_dev.data_ptr(), self._img_dev.data_ptr(), self._chunks_dev.data_ptr(),
                  self._n_chunks, self._partial_dev.data_ptr(), self.scalars.data_ptr(), self._groups_dev_addr,
                  self._img_groups_addr[k], len(self.param_groups), float(self.max_grad_norm), _lib.stream_of(self._img_dev))
        self._keep = keep  # conforming copies stay alive until the next step (the kernels read them asynchronously)

    def zero_grad(self):
        for p in self.low:
            p.grad = None
        for p in self.other:
            p.grad = None

    @torch.no_grad()
    def step(self):
        self._update()
        self.opt._opt_called = True   # what torch's schedulers look for: the flat and direct paths do not call self.opt.step()
        if self.transposed is not None:
            self.transposed.refresh()

    def _update(self):
        if self.flat:
            return self._step_flat()
        have = [(m.grad, p.grad) for m, p in zip(self.master, self.low) if p.grad is not None]
        if have:
            torch._foreach_copy_([a for a, _ in have], [b for _, b in have])  # bf16 -> fp32, one multi-tensor kernel
        if len(have) != len(self.low):
            # a parameter unused in this step: zero gradient, as the flat all-reduce path produces at world size > 1
            # (grad_sync.FlatGradAllReduce zero-fills), so the update does not depend on the world size.  Deviation from
            # torch.optim (and the reference's optimizer), which SKIP a parameter without a gradient: here it still gets its
            # weight decay and moment decay -- for every parameter kind alike (bf16-with-master and fp32)
            torch._foreach_zero_([m.grad for m, p in zip(self.master, self.low) if p.grad is None])
        for p in self.other:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        if self.direct:
            grads = [p.grad for p in self._params]
            found_inf = None
            if self.max_grad_norm is not None:
                # clip_grad_norm_(foreach=True): per-tensor 2-norms in one multi-tensor launch, the norm of the norms, one scale
                total = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads, 2.0)), 2.0)
                torch._foreach_mul_(grads, torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0))
                found_inf = (~torch.isfinite(total)).to(torch.float32)
            self._steps_flat.add_(1)
            for g, idx, (params, exp_avg, exp_avg_sq, steps) in zip(self.param_groups, self._group_idx, self._direct_groups):
                torch._fused_adamw_(params, [grads[i] for i in idx], exp_avg, exp_avg_sq, [], steps, amsgrad=False, maximize=False,
                                    grad_scale=None, found_inf=found_inf, lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1],
                                    weight_decay=g["weight_decay"], eps=g["eps"])
            if found_inf is not None:
                self._steps_flat.sub_(found_inf)   # a skipped step does not advance the bias correction
        else:
            if self.max_grad_norm is not None:
                norm = torch.nn.utils.clip_grad_norm_(self.master + self.other, self.max_grad_norm, foreach=True)
                skip_nonfinite_step(self.opt, norm)
            self.opt.step()
        torch._foreach_copy_(self.low, self.master)                  # fp32 -> bf16

    # ------------------------------------------------------------------ checkpoints
    def _moments(self):
        """(first moments, second moments, step) in the order of `master + other`; step is a host number (one device read)."""
        params = self.master + self.other
        if self.flat:
            return self._flat_m, self._flat_v, float(self.scalars[2])
        if self.direct:
            return self._exp_avg, self._exp_avg_sq, float(self._steps_flat[0]) if params else 0.0
        st = [self.opt.state.get(p) for p in params]
        zeros = lambda p: torch.zeros_like(p, memory_format=torch.preserve_format)  # noqa: E731  (torch creates them at its first step)
        steps = {float(s["step"]) for s in st if s}
        assert len(steps) <= 1, steps
        return ([s["exp_avg"] if s else zeros(p) for s, p in zip(st, params)],
                [s["exp_avg_sq"] if s else zeros(p) for s, p in zip(st, params)], steps.pop() if steps else 0.0)

    @torch.no_grad()
    def state_dict(self):
        """{"state": {i: {"step", "exp_avg", "exp_avg_sq"}} as torch.optim.AdamW writes it, i in self.opt's parameter order (the
        groups one after another); "param_groups": as torch writes them; "master": the fp32 masters of `self.low`, in order}.
        Copies, on the tensors' device; the same layout from the flat, the direct and the object path."""
        m, v, step = self._moments()
        state = {j: dict(step=torch.tensor(step, dtype=torch.float32), exp_avg=m[i].detach().clone(), exp_avg_sq=v[i].detach().clone())
                 for j, i in enumerate(self._opt_order)}
        return dict(state=state, param_groups=self.opt.state_dict()["param_groups"], master=[x.detach().clone() for x in self.master])

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Restore what `state_dict()` wrote, from any of the three paths.  Everything is copied IN PLACE: masters, moments
        and group dicts keep their identity, so the device addresses in the flat tables, `self.param_groups` and a scheduler
        built on `self.opt` stay valid.  The bf16 parameters are rounded from the restored masters and the transposed weight
        copies rebuilt.  This optimizer has ONE step counter: a state whose per-parameter steps differ raises ValueError."""
        params = self.master + self.other
        state, groups, master = state_dict["state"], state_dict["param_groups"], state_dict["master"]
        if len(state) != len(params) or len(master) != len(self.master) or len(groups) != len(self.param_groups) or any(
                len(g["params"]) != len(idx) for g, idx in zip(groups, self._group_idx)):
            raise ValueError("optimizer state does not fit: %d states / %d masters / groups of %s here, %d / %d / %s in the state" % (
                len(params), len(self.master), [len(i) for i in self._group_idx], len(state), len(master),
                [len(g["params"]) for g in groups]))
        steps = sorted({float(s["step"]) for s in state.values()})
        if len(steps) > 1:
            raise ValueError("optimizer state with unequal per-parameter steps %s: MasterWeightAdamW keeps one step counter for all "
                             "parameters (torch skips parameters without a gradient; here they get a zero gradient)" % steps[:4])
        step = steps[0] if steps else 0.0
        for j, i in enumerate(self._opt_order):
            for key in ("exp_avg", "exp_avg_sq"):
                if state[j][key].shape != params[i].shape:
                    raise ValueError("optimizer state %d: %s has shape %s, the parameter %s" % (
                        j, key, tuple(state[j][key].shape), tuple(params[i].shape)))
        for g, src in zip(self.param_groups, groups):
            g.update({k: v for k, v in src.items() if k != "params"})
        if not (self.flat or self.direct):
            for p in params:     # torch creates a parameter's state at its first step
                if not self.opt.state.get(p):
                    self.opt.state[p] = dict(step=torch.zeros((), dtype=torch.float32, device=p.device),
                                             exp_avg=torch.zeros_like(p, memory_format=torch.preserve_format),
                                             exp_avg_sq=torch.zeros_like(p, memory_format=torch.preserve_format))
                self.opt.state[p]["step"].fill_(step)
        m, v, _ = self._moments()
        for j, i in enumerate(self._opt_order):
            m[i].copy_(state[j]["exp_avg"])
            v[i].copy_(state[j]["exp_avg_sq"])
        if self.flat:
            self.scalars[2] = step
        elif self.direct:
            self._steps_flat.fill_(step)
        for dst, src in zip(self.master, master):
            dst.copy_(src)
        if self.low:
            torch._foreach_copy_(self.low, self.master)                  # fp32 -> bf16
        if self.transposed is not None:
            self.transposed.refresh()
