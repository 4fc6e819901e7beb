"""Swin Transformer image backbone (`img_backbone = mmdet.SwinTransformer` of the reference's camera configs,
projects/BEVFusion/configs/nuscenes/bevfusion_lidar-cam_voxel0075_second_secfpn_8xb4-cyclic-20e_nus-3d.py:15-35).

mmdet is an external dependency of the reference and is not vendored there, so the module tree and the state-dict names
below are written from knowledge of mmdet 3.x (`mmdet/models/backbones/swin.py`): parity with it is unpinned, as for the
sparse encoder.  All names live in this one file.

Activations are [B, H, W, C] throughout (what the Linears and LayerNorms want); the stage outputs are returned as
[B, C, H, W] VIEWS of that memory, i.e. channels-last maps without a copy.

Attention runs in csrc/swin_attn.hip when it can: the qkv Linear's output goes into the kernel as it is, and the cyclic
shift, window partition, bias, mask and softmax happen there.  Everything else (CPU, fp32, attention dropout in training,
other window or head sizes, BFHIP_SWIN_ATTN=0) takes the plain-torch path of the published algorithm.

With BFHIP_SWIN_LN=1 (layernorm.ENABLED; it ships off) the token-wise glue runs in csrc/layernorm.hip
(layernorm.py) on the GPU: a block is LayerNorm, then residual add + drop path +
LayerNorm in one launch, then residual add + drop path, three launches over the fp32 stream instead of eight library kernels;
the patch-embedding, patch-merging and output norms use the same kernel.  The switch off, the CPU, or an
autocast dtype other than bf16 keep the nn.LayerNorm modules and torch adds.  Module tree, parameters and state-dict keys are
the same either way.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.checkpoint import checkpoint

from . import _lib, layernorm
from .linear_rows import linear_rows
from .registry import MODELS

HIP_WINDOW = 7
HIP_HEAD_DIM = 32
ENABLED = os.environ.get("BFHIP_SWIN_ATTN", "1") != "0"


# ------------------------------------------------------------------------------------------------ kernel front-end
class _WindowAttentionFn(torch.autograd.Function):
    """qkv bf16 [B, Hp, Wp, 3C] (token pitch >= 3C), bias f32 [heads, 49, 49] -> out bf16 [B, Hp, Wp, C]."""

    @staticmethod
    def forward(ctx, qkv, bias, heads, shift, scale):
        B, Hp, Wp, C3 = qkv.shape
        pitch = qkv.stride(2)
        if (qkv.stride(3) != 1 or qkv.stride(1) != Wp * pitch or qkv.stride(0) != Hp * Wp * pitch or pitch % 8
                or qkv.data_ptr() % 16):
            qkv = qkv.contiguous()
            pitch = C3
        bias = bias.contiguous()
        C = C3 // 3
        out = torch.empty((B, Hp, Wp, C), dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty((B, Hp, Wp, heads), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.call("bfhip_swin_attn_fwd", qkv.data_ptr(), pitch, bias.data_ptr(), B, Hp, Wp, heads, shift, scale,
                      out.data_ptr(), lse.data_ptr(), _lib.stream_of(qkv))
        ctx.save_for_backward(qkv, bias, out, lse)
        ctx.cfg = (heads, shift, scale, pitch)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, bias, out, lse = ctx.saved_tensors
        heads, shift, scale, pitch = ctx.cfg
        B, Hp, Wp, C3 = qkv.shape
        dout = dout.to(torch.bfloat16).contiguous()
        dqkv = torch.empty((B, Hp, Wp, C3), dtype=torch.bfloat16, device=qkv.device)
        parts = _lib.load().bfhip_swin_attn_parts(B, Hp, Wp, heads)
        partial = torch.empty((parts, heads, 49, 49), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.call("bfhip_swin_attn_bwd", qkv.data_ptr(), pitch, bias.data_ptr(), out.data_ptr(), dout.data_ptr(),
                      lse.data_ptr(), B, Hp, Wp, heads, shift, scale, dqkv.data_ptr(), partial.data_ptr(), parts,
                      _lib.stream_of(qkv))
        ctx.partial = partial  # kept for the reproducibility test
        dbias = partial.sum(0) if ctx.needs_input_grad[1] else None  # a fixed-order reduction
        return dqkv, dbias, None, None, None


def window_attention(qkv, bias, heads, shift, scale=None):
    """Fused shifted-window attention (csrc/swin_attn.hip).  A shape or dtype the kernels do not cover is an error."""
    B, Hp, Wp, C3 = qkv.shape
    C = C3 // 3
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and C3 == 3 * C and C % heads == 0 and bias.dtype == torch.float32
            and tuple(bias.shape) == (heads, 49, 49)
            and _lib.load().bfhip_swin_attn_supported(B, Hp, Wp, heads, HIP_WINDOW, C // heads, shift)):
        raise RuntimeError("window_attention: unsupported input (bf16 [B, Hp, Wp, 3 * heads * 32] on the GPU, Hp and Wp "
                           "multiples of 7, shift 0 or 3, f32 bias [heads, 49, 49])")
    return _WindowAttentionFn.apply(qkv, bias, heads, int(shift), float(scale if scale is not None else (C // heads) ** -0.5))


class _BiasGatherFn(torch.autograd.Function):
    """bias[h, i, j] = table[index[i, j], h].  The backward adds the <= 49 pairs of every table row through a fixed
    gather plan and a row sum instead of an atomic index-add: run-to-run reproducible."""

    @staticmethod
    def forward(ctx, table, index, plan):
        n = index.shape[0]
        ctx.save_for_backward(plan)
        ctx.table_dtype = table.dtype
        return table[index.reshape(-1)].float().t().reshape(table.shape[1], n, index.shape[1]).contiguous()

    @staticmethod
    def backward(ctx, g):
        (plan,) = ctx.saved_tensors
        heads = g.shape[0]
        flat = torch.cat([g.reshape(heads, -1).float(), g.new_zeros((heads, 1), dtype=torch.float32)], 1)
        dt = flat[:, plan.reshape(-1)].reshape(heads, plan.shape[0], plan.shape[1]).sum(-1)  # [heads, rows]
        return dt.t().contiguous().to(ctx.table_dtype), None, None


def gather_plan(index, rows):
    """i64 [rows, m]: for every table row the positions of `index` (flattened) that read it, padded with numel (a zero slot)."""
    flat = index.reshape(-1)
    n = flat.numel()
    order = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=rows)
    starts = torch.cumsum(counts, 0) - counts
    m = max(int(counts.max()), 1)
    plan = torch.full((rows, m), n, dtype=torch.long, device=index.device)
    srt = flat[order]
    plan[srt, torch.arange(n, device=index.device) - starts[srt]] = order
    return plan


def drop_path(x, p, training):
    """Stochastic depth per sample: zero the whole sample with probability p, scale the others by 1 / (1 - p)."""
    if p == 0.0 or not training:
        return x
    keep = 1.0 - p
    mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
    return x * (mask / keep)


def drop_path_scale(x, p, training):
    """The per-sample factor drop_path(x, p, training) multiplies by, as f32 [B], or None where drop_path is the identity.  The
    mask is drawn by the same call with the same shape and dtype, so a seeded run drops the same samples either way."""
    if p == 0.0 or not training:
        return None
    keep = 1.0 - p
    mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
    return (mask / keep).reshape(-1).float()


def _ln_kernel_path(x):
    """Do the LayerNorms and residual adds around x go through layernorm.py?  (It still falls back per call for what the kernels
    do not cover.)  Off: exactly the module calls and torch arithmetic of the plain path."""
    if not (layernorm.ENABLED and x.is_cuda):
        return False
    return not torch.is_autocast_enabled("cuda") or torch.get_autocast_dtype("cuda") == torch.bfloat16


def _norm(ln, x, to_linear=False):
    """nn.LayerNorm `ln` over x [..., C].  On the kernel path the output has the dtype its consumer sees today: fp32 under
    autocast (x's dtype without), or, where the consumer is a Linear (`to_linear`), the bf16 that autocast casts it to."""
    if not (_ln_kernel_path(x) and ln.elementwise_affine and ln.bias is not None and len(ln.normalized_shape) == 1):
        return ln(x)
    if torch.is_autocast_enabled("cuda"):
        out = torch.bfloat16 if to_linear else torch.float32
    else:
        out = x.dtype
    return layernorm.layer_norm_rows(x, ln.weight, ln.bias, ln.eps, out)


def _rows(lin, x):
    """nn.Linear over the last axis of [.., C] through linear_rows ([tokens, C] matrix: split-K weight gradient)."""
    return linear_rows(x.reshape(-1, x.shape[-1]), lin.weight, lin.bias).view(*x.shape[:-1], lin.out_features)


# ------------------------------------------------------------------------------------------------ modules (mmdet 3.x names)
class WindowMSA(nn.Module):
    def __init__(self, embed_dims, num_heads, window_size, qkv_bias=True, qk_scale=None, attn_drop_rate=0.0, proj_drop_rate=0.0):
        super().__init__()
        self.embed_dims, self.num_heads, self.window_size = embed_dims, num_heads, window_size
        self.scale = qk_scale or (embed_dims // num_heads) ** -0.5
        ws = window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) * (2 * ws - 1), num_heads))
        ys, xs = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
        ys, xs = ys.reshape(-1), xs.reshape(-1)
        index = (ys[:, None] - ys[None, :] + ws - 1) * (2 * ws - 1) + (xs[:, None] - xs[None, :] + ws - 1)
        self.register_buffer("relative_position_index", index.contiguous())  # persistent: a checkpoint's buffer wins
        self.qkv = nn.Linear(embed_dims, embed_dims * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop_rate)
        self.proj = nn.Linear(embed_dims, embed_dims)
        self.proj_drop = nn.Dropout(proj_drop_rate)
        self.softmax = nn.Softmax(dim=-1)
        self._plan = None
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def dense_bias(self):
        """f32 [heads, N, N] = table[index]; the table's gradient comes back through a fixed-order gather."""
        index = self.relative_position_index
        key = (index.device, index._version, index.data_ptr())
        if self._plan is None or self._plan[0] != key:
            self._plan = (key, gather_plan(index, self.relative_position_bias_table.shape[0]))
        return _BiasGatherFn.apply(self.relative_position_bias_table, index, self._plan[1])

    def forward(self, x, mask=None):
        """x [windows * B, N, C], mask [windows, N, N] or None: the published window attention, plain torch."""
        B_, N, C = x.shape
        qkv = self.qkv(x).reshape(B_, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * self.scale, qkv[1], qkv[2]
        attn = q @ k.transpose(-2, -1)
        attn = attn + self.dense_bias().to(attn.dtype).unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            attn = attn.view(B_ // nW, nW, self.num_heads, N, N) + mask.to(attn.dtype).unsqueeze(1).unsqueeze(0)
            attn = attn.view(-1, self.num_heads, N, N)
        attn = self.attn_drop(self.softmax(attn))
        x = (attn @ v).transpose(1, 2).reshape(B_, N, C)
        return self.proj_drop(self.proj(x))


class ShiftWindowMSA(nn.Module):
    def __init__(self, embed_dims, num_heads, window_size, shift_size=0, qkv_bias=True, qk_scale=None, attn_drop_rate=0.0,
                 proj_drop_rate=0.0, drop_path_rate=0.0):
        super().__init__()
        assert 0 <= shift_size < window_size
        self.window_size, self.shift_size = window_size, shift_size
        self.attn_drop_rate, self.drop_path_rate = attn_drop_rate, drop_path_rate
        self.w_msa = WindowMSA(embed_dims, num_heads, window_size, qkv_bias, qk_scale, attn_drop_rate, proj_drop_rate)

    def hip_eligible(self, x):
        w = self.w_msa
        if not (ENABLED and x.is_cuda and self.window_size == HIP_WINDOW and w.embed_dims == w.num_heads * HIP_HEAD_DIM
                and self.shift_size in (0, 3) and (self.attn_drop_rate == 0.0 or not self.training)):
            return False
        if torch.is_autocast_enabled("cuda"):
            return torch.get_autocast_dtype("cuda") == torch.bfloat16
        return x.dtype == torch.bfloat16

    def forward(self, x):
        """x [B, H, W, C] (the LayerNorm's output) -> attention output [B, H, W, C], drop path applied."""
        return drop_path(self.branch(x), self.drop_path_rate, self.training)

    def branch(self, x):
        """forward() before its drop path (SwinBlock hands the drop-path factor to the residual kernel instead)."""
        return self._forward_hip(x) if self.hip_eligible(x) else self._forward_torch(x)

    def _forward_hip(self, x):
        B, H, W, C = x.shape
        ws, w = self.window_size, self.w_msa
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        with torch.autocast("cuda", dtype=torch.bfloat16):
            x = x.to(torch.bfloat16)
            if (Hp, Wp) != (H, W):
                x = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))  # padded tokens still pass the qkv Linear: q = k = v = bias
            qkv = _rows(w.qkv, x)
            out = window_attention(qkv, w.dense_bias(), w.num_heads, self.shift_size, w.scale)
            if (Hp, Wp) != (H, W):
                out = out[:, :H, :W]
            return w.proj_drop(_rows(w.proj, out))

    def _forward_torch(self, x):
        B, H, W, C = x.shape
        ws, s = self.window_size, self.shift_size
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        x = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))
        mask = None
        if s > 0:
            x = torch.roll(x, shifts=(-s, -s), dims=(1, 2))
            img = torch.zeros((1, Hp, Wp, 1), device=x.device)
            cnt = 0
            for hs in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                for wsl in (slice(0, -ws), slice(-ws, -s), slice(-s, None)):
                    img[:, hs, wsl, :] = cnt
                    cnt += 1
            mw = self._partition(img).reshape(-1, ws * ws)
            mask = mw.unsqueeze(1) - mw.unsqueeze(2)
            mask = mask.masked_fill(mask != 0, -100.0)
        wins = self._partition(x).reshape(-1, ws * ws, C)
        out = self.w_msa(wins, mask).view(-1, ws, ws, C)
        out = out.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
        if s > 0:
            out = torch.roll(out, shifts=(s, s), dims=(1, 2))
        return out[:, :H, :W].contiguous()

    def _partition(self, x):
        B, H, W, C = x.shape
        ws = self.window_size
        return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws, ws, C)


class SwinFFN(nn.Module):
    """mmcv FFN with GELU: keys `layers.0.0.*`, `layers.1.*`; the identity is added by the block."""

    def __init__(self, embed_dims, feedforward_channels, ffn_drop=0.0):
        super().__init__()
        self.layers = nn.Sequential(
            nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.GELU(), nn.Dropout(ffn_drop)),
            nn.Linear(feedforward_channels, embed_dims), nn.Dropout(ffn_drop))

    def forward(self, x):
        fc1, act, d1 = self.layers[0]
        return self.layers[2](_rows(self.layers[1], d1(act(_rows(fc1, x)))))


class SwinBlock(nn.Module):
    def __init__(self, embed_dims, num_heads, feedforward_channels, window_size=7, shift=False, qkv_bias=True, qk_scale=None,
                 drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.0, with_cp=False):
        super().__init__()
        self.with_cp, self.drop_path_rate = with_cp, drop_path_rate
        self.norm1 = nn.LayerNorm(embed_dims)
        self.attn = ShiftWindowMSA(embed_dims, num_heads, window_size, window_size // 2 if shift else 0, qkv_bias, qk_scale,
                                   attn_drop_rate, drop_rate, drop_path_rate)
        self.norm2 = nn.LayerNorm(embed_dims)
        self.ffn = SwinFFN(embed_dims, feedforward_channels, drop_rate)

    def _inner(self, x):
        n1, n2 = self.norm1, self.norm2
        if not (_ln_kernel_path(x) and n1.elementwise_affine and n2.elementwise_affine and n1.bias is not None and n2.bias is not None):
            x = x + self.attn(self.norm1(x))
            return x + drop_path(self.ffn(self.norm2(x)), self.drop_path_rate, self.training)
        # three launches of csrc/layernorm.hip; the masks are drawn where drop_path drew them (after each branch is computed)
        ydt = torch.bfloat16 if torch.is_autocast_enabled("cuda") else x.dtype  # what the qkv / fc1 Linear sees today
        a = self.attn.branch(layernorm.layer_norm_rows(x, n1.weight, n1.bias, n1.eps, ydt))
        x, y = layernorm.add_layer_norm_rows(x, a, drop_path_scale(a, self.drop_path_rate, self.training), n2.weight, n2.bias,
                                             n2.eps, ydt)
        f = self.ffn(y)
        return layernorm.scaled_add_rows(x, f, drop_path_scale(f, self.drop_path_rate, self.training))

    def forward(self, x):
        if self.with_cp and x.requires_grad:
            return checkpoint(self._inner, x, use_reentrant=False)
        return self._inner(x)


class PatchMerging(nn.Module):
    """2 x 2 neighbours concatenated in nn.Unfold's channel order (c * 4 + kh * 2 + kw), LayerNorm, Linear(4C, 2C)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.norm = nn.LayerNorm(4 * in_channels)
        self.reduction = nn.Linear(4 * in_channels, out_channels, bias=False)

    @staticmethod
    def gather(x):
        B, H, W, C = x.shape
        if H % 2 or W % 2:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
            H, W = H + H % 2, W + W % 2
        return x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, 4 * C)

    def forward(self, x):
        return _rows(self.reduction, _norm(self.norm, self.gather(x), to_linear=True))


class SwinBlockSequence(nn.Module):
    def __init__(self, embed_dims, num_heads, feedforward_channels, depth, window_size, qkv_bias, qk_scale, drop_rate,
                 attn_drop_rate, drop_path_rates, downsample, with_cp):
        super().__init__()
        self.blocks = nn.ModuleList(
            SwinBlock(embed_dims, num_heads, feedforward_channels, window_size, i % 2 == 1, qkv_bias, qk_scale, drop_rate,
                      attn_drop_rate, drop_path_rates[i], with_cp) for i in range(depth))
        self.downsample = downsample

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        return (self.downsample(x) if self.downsample is not None else x), x


class PatchEmbed(nn.Module):
    def __init__(self, in_channels, embed_dims, patch_size, stride, norm):
        super().__init__()
        self.patch_size = patch_size
        self.projection = nn.Conv2d(in_channels, embed_dims, patch_size, stride=stride)
        self.norm = nn.LayerNorm(embed_dims) if norm else None

    def forward(self, x):
        ps = self.patch_size
        H, W = x.shape[2:]
        if H % ps or W % ps:
            x = F.pad(x, (0, -W % ps, 0, -H % ps))
        if x.is_cuda:
            x = x.contiguous(memory_format=torch.channels_last)  # the permute below is then the map's own memory order
        x = self.projection(x).permute(0, 2, 3, 1)
        return _norm(self.norm, x) if self.norm is not None else x.contiguous()


class SwinTransformer(nn.Module):
    """mmdet.SwinTransformer with the arguments of the reference's config.  `init_cfg` and `convert_weights` are stored and
    nothing is fetched; converting the keys of an original-format checkpoint is not done here.

    `frozen_stages` follows mmdet 3.x's `_freeze_stages` from knowledge of that package (parity unpinned, like the rest of the
    file): with frozen_stages >= 0 the patch embedding and `drop_after_pos` go to eval with requires_grad off; for i in
    1 .. frozen_stages so do `stages[i - 1]` (its patch merging included) and `norm{i-1}` when that index is an output.  train()
    re-applies it, so a frozen part stays in eval."""

    def __init__(self, pretrain_img_size=224, in_channels=3, embed_dims=96, patch_size=4, window_size=7, mlp_ratio=4,
                 depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), strides=(4, 2, 2, 2), out_indices=(0, 1, 2, 3), qkv_bias=True,
                 qk_scale=None, patch_norm=True, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.1, use_abs_pos_embed=False,
                 with_cp=False, pretrained=None, convert_weights=False, frozen_stages=-1, init_cfg=None):
        super().__init__()
        assert strides[0] == patch_size, "the patch embedding's stride is the patch size"
        assert not use_abs_pos_embed, "absolute position embedding is not built (no reference config uses it)"
        assert tuple(strides[1:]) == (2,) * (len(depths) - 1), "patch merging is 2 x 2"
        assert -1 <= frozen_stages <= len(depths), "frozen_stages counts stages"
        self.frozen_stages = frozen_stages
        self.convert_weights, self.init_cfg, self.pretrained = convert_weights, init_cfg, pretrained
        self.out_indices = tuple(out_indices)
        self.patch_embed = PatchEmbed(in_channels, embed_dims, patch_size, strides[0], patch_norm)
        self.drop_after_pos = nn.Dropout(drop_rate)
        total = sum(depths)
        dpr = [drop_path_rate * i / max(total - 1, 1) for i in range(total)]  # linear, 0 .. drop_path_rate over all blocks
        self.stages = nn.ModuleList()
        self.num_features = []
        c = embed_dims
        for i, depth in enumerate(depths):
            down = PatchMerging(c, 2 * c) if i < len(depths) - 1 else None
            self.stages.append(SwinBlockSequence(c, num_heads[i], int(mlp_ratio * c), depth, window_size, qkv_bias, qk_scale,
                                                 drop_rate, attn_drop_rate, dpr[sum(depths[:i]):sum(depths[:i + 1])], down,
                                                 with_cp))
            self.num_features.append(c)
            c = 2 * c
        for i in self.out_indices:
            self.add_module("norm%d" % i, nn.LayerNorm(self.num_features[i]))
        self.apply(self._init)
        self._freeze_stages()

    def _freeze_stages(self):
        def freeze(m):
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

        if self.frozen_stages >= 0:
            freeze(self.patch_embed)
            self.drop_after_pos.eval()
        for i in range(1, self.frozen_stages + 1):
            if i - 1 in self.out_indices:
                freeze(getattr(self, "norm%d" % (i - 1)))
            freeze(self.stages[i - 1])

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self

    @staticmethod
    def _init(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.LayerNorm):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.drop_after_pos(self.patch_embed(x))
        outs = []
        for i, stage in enumerate(self.stages):
            x, out = stage(x)
            if i in self.out_indices:
                outs.append(_norm(getattr(self, "norm%d" % i), out).permute(0, 3, 1, 2))  # [B, C, H, W] view: channels-last
        return tuple(outs)


MODELS.register_module(name="SwinTransformer", module=SwinTransformer)
MODELS.register_module(name="mmdet.SwinTransformer", module=SwinTransformer)


def swin_t_config():
    """The backbone dict of the reference's camera configs (the checkpoint URL of its init_cfg is kept as data: nothing is
    fetched)."""
    return dict(type="mmdet.SwinTransformer", embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7,
                mlp_ratio=4, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.2,
                patch_norm=True, out_indices=[1, 2, 3], with_cp=False, convert_weights=True,
                init_cfg=dict(type="Pretrained", checkpoint="swin_tiny_patch4_window7_224.pth"))
