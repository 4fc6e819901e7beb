"""Inputs and restatements shared by tests/test_query_init_cpu.py and tests/test_query_init_gpu.py.

Score maps without ties: per sample a seeded random permutation of (i + 1) / (N + 1), i < N = C*H*W.  All N values are distinct
in float32 (their spacing, 1 / (N + 1) >= 3e-6, is far above the float32 spacing below 1), so torch.topk is unambiguous on them.
About one interior cell in nine is the maximum of its 3x3 window."""
import functools

import torch
import torch.nn.functional as F

# (B, C, H, W, K)
SHAPES = [(2, 3, 20, 24, 50), (3, 10, 48, 64, 200), (1, 5, 40, 40, 500), (2, 10, 180, 180, 200)]
SMALL, MID, DUPS, FULL = SHAPES
SHORT = (1, 2, 8, 8, 40)   # about 8 positive peaks: fewer than K
CH = 24                    # feature channels: 3 (bf16) or 6 (f32) 16-byte vectors a row, neither a power of two


@functools.lru_cache(maxsize=None)
def distinct_map(shape, seed=0):
    B, C, H, W, _ = shape
    N = C * H * W
    g = torch.Generator().manual_seed(1000 + seed)
    vals = ((torch.arange(N, dtype=torch.float64) + 1) / (N + 1)).float()
    assert torch.unique(vals).numel() == N
    return torch.stack([vals[torch.randperm(N, generator=g)] for _ in range(B)]).view(B, C, H, W)


@functools.lru_cache(maxsize=None)
def features(shape, seed=0):
    """[B, HW, CH] f32: `features(...).transpose(1, 2)` is `flat` as the channels-last view the shared conv produces."""
    B, _, H, W, _ = shape
    return torch.randn(B, H * W, CH, generator=torch.Generator().manual_seed(2000 + seed))


def bev_pos(H, W):
    """BEVFusionHead's buffer for an H x W map (dense_modules.BEVFusionHead.__init__)."""
    bx, by = torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), indexing="ij")
    return torch.stack([bx + 0.5, by + 0.5], 0).view(1, 2, -1).permute(0, 2, 1)


def parent_chain(h, flat, K, pos):
    """The torch ops of BEVFusionHead.forward between the sigmoid and the decoder, as they stood before query_init."""
    B, C = h.shape[:2]
    heatmap = h
    pad = 1
    local_max = torch.zeros_like(heatmap)
    inner = F.max_pool2d(heatmap, kernel_size=3, stride=1, padding=0)
    local_max[:, :, pad:-pad, pad:-pad] = inner
    heatmap = (heatmap * (heatmap == local_max)).reshape(B, heatmap.shape[1], -1)
    top = heatmap.reshape(B, -1).topk(K, dim=-1).indices
    top_class, top_index = top // heatmap.shape[-1], top % heatmap.shape[-1]
    rows = flat.transpose(1, 2)[torch.arange(B, device=flat.device)[:, None], top_index]
    query_pos = pos.expand(B, -1, -1).gather(index=top_index[:, :, None].expand(-1, -1, 2), dim=1)
    score = heatmap.gather(index=top_index[:, None, :].expand(-1, C, -1), dim=-1)
    return top_class, top_index, query_pos, score, rows


def positive_peaks(h):
    """Per sample: the number of cells the parent chain leaves positive."""
    local_max = torch.zeros_like(h)
    local_max[:, :, 1:-1, 1:-1] = F.max_pool2d(h, kernel_size=3, stride=1, padding=0)
    return ((h * (h == local_max)) > 0).flatten(1).sum(1)


def shared_cells(top_index):
    """Picks that land on a cell an earlier pick of the sample already took."""
    return sum(int(row.numel() - torch.unique(row).numel()) for row in top_index)


def ordered_backward(top_index, d_rows, HW):
    """d_flat [B, HW, Ch]: an f32 loop over the picks in ascending p, rounded once to d_rows' dtype."""
    B, K, Ch = d_rows.shape
    acc = torch.zeros(B, HW, Ch, dtype=torch.float32)
    idx, g = top_index.cpu(), d_rows.detach().float().cpu()
    for b in range(B):
        for p in range(K):
            acc[b, idx[b, p]] += g[b, p]
    return acc.to(d_rows.dtype)


def eighths_map(shape, seed=0):
    B, C, H, W, _ = shape
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.floor(torch.rand(B, C, H, W, generator=g) * 8) / 8


def tie_cases():
    """name -> (h, K): plateaus, shortfalls and NaNs, where only the defined order decides."""
    cases = {}
    for name, shape in (("small", SMALL), ("mid", MID)):
        B, C, H, W, K = shape
        cases["eighths_" + name] = (eighths_map(shape), K)
        cases["zeros_" + name] = (torch.zeros(B, C, H, W), K)
        cases["constant_" + name] = (torch.full((B, C, H, W), 0.5), K)
    cases["short"] = (distinct_map(SHORT), SHORT[4])
    nan = distinct_map(SHORT, seed=1).clone()
    nan[0, 0, 3, 4] = nan[0, 1, 0, 0] = nan[0, 1, 7, 2] = float("nan")
    cases["short_nan"] = (nan, SHORT[4])
    nan2 = distinct_map(SMALL, seed=1).clone()
    nan2[0, 1, 5, 5] = nan2[1, 2, 10, 3] = float("nan")
    cases["nan"] = (nan2, SMALL[4])
    return cases


def assert_same(got, want, what=""):
    names = ("top_class", "top_index", "query_pos", "query_heatmap_score", "rows")
    for name, a, b in zip(names, got, want):
        a, b = a.detach().cpu(), b.detach().cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        assert torch.equal(a, b), (what, name, int((a != b).sum()))
