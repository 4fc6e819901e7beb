"""CPU: the arithmetic of query initialisation (bevfusion_amd/query_init.py::torch_query_init) against the torch chain
BEVFusionHead.forward ran before it, and its defined order where torch.topk has none.  Everything is compared bit for bit."""
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import query_init as qi
from bevfusion_amd.dense_modules import BEVFusionHead
import query_init_cases as qc


def inputs(shape, seed=0):
    B, C, H, W, K = shape
    return qc.distinct_map(shape, seed), qc.features(shape, seed).transpose(1, 2), K, qc.bev_pos(H, W), W


@pytest.mark.parametrize("shape", qc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_query_init_is_the_parent_chain(shape):
    h, flat, K, pos, W = inputs(shape)
    peaks = qc.positive_peaks(h)
    print("positive peaks per sample", peaks.tolist())
    assert int(peaks.min()) >= K
    want = qc.parent_chain(h, flat, K, pos)
    qc.assert_same(qi.torch_query_init(h, flat, K, W), want, str(shape))
    print("picks on an already picked cell:", qc.shared_cells(want[1]))


def test_third_shape_has_many_shared_cells():
    h, flat, K, pos, W = inputs(qc.DUPS)
    shared = qc.shared_cells(qi.torch_query_init(h, flat, K, W)[1])
    print("picks on an already picked cell:", shared)
    assert shared >= 40


def brute_force_order(h, K, nms_free=()):
    """(m descending, flat index ascending) by a Python sort of every cell; NaN cells last."""
    B, C, H, W = h.shape
    m = qi.masked_scores(h, nms_free)
    out = []
    for b in range(B):
        hv, mv = h[b].flatten().tolist(), m[b].flatten().tolist()
        key = [(1, 0.0, i) if hv[i] != hv[i] else (0, -mv[i], i) for i in range(len(hv))]
        out.append([k[2] for k in sorted(key)[:K]])
    return torch.tensor(out)


@pytest.mark.parametrize("name", ["eighths_small", "zeros_small", "constant_small", "short", "short_nan", "nan"])
def test_tie_rule_and_fill(name):
    h, K = qc.tie_cases()[name]
    B, C, H, W = h.shape
    flat = torch.randn(B, 8, H * W, generator=torch.Generator().manual_seed(5))
    top_class, top_index, query_pos, score, rows = qi.torch_query_init(h, flat, K, W)
    want = brute_force_order(h, K)
    assert torch.equal(top_class * (H * W) + top_index, want)
    m = qi.masked_scores(h).reshape(B, C, H * W)
    picked = m.reshape(B, -1).gather(1, want)
    assert not torch.isnan(picked).any() and (picked[:, 1:] <= picked[:, :-1]).all()
    if name.startswith("zeros"):
        assert torch.equal(want, torch.arange(K).expand(B, K))
    if name.startswith("constant"):   # class 0's interior cells in row-major order
        first = torch.tensor([y * W + x for y in range(1, H - 1) for x in range(1, W - 1)][:K])
        assert torch.equal(want, first.expand(B, K))
    if name.startswith("short"):
        n = int((m[0] > 0).sum())
        assert 0 < n < K and (picked[0, :n] > 0).all() and (picked[0, n:] == 0).all()
        tail = want[0, n:]
        assert (tail[1:] > tail[:-1]).all(), "the zero cells follow in ascending flat index"
        assert not torch.isnan(h.flatten()[tail]).any(), "a NaN score is never picked"
    assert torch.equal(score, m.gather(2, top_index[:, None, :].expand(-1, C, -1)))


def test_nms_free_classes_against_explicit_restatement():
    h, flat, K, pos, W = inputs(qc.SMALL)
    B, C, H, _ = h.shape
    local_max = torch.zeros_like(h)
    local_max[:, :, 1:-1, 1:-1] = torch.nn.functional.max_pool2d(h, 3, 1, 0)
    local_max[:, 1] = h[:, 1]
    m = (h * (h == local_max)).reshape(B, C, -1)
    top = m.reshape(B, -1).topk(K, dim=-1).indices   # distinct scores: unambiguous
    got = qi.torch_query_init(h, flat, K, W, nms_free_classes=(1,))
    assert torch.equal(got[0], top // (H * W)) and torch.equal(got[1], top % (H * W))
    assert torch.equal(got[3], m.gather(2, got[1][:, None, :].expand(-1, C, -1)))
    assert int((got[0] == 1).sum()) > int((qi.torch_query_init(h, flat, K, W)[0] == 1).sum())
    border = (got[1] // W == 0) | (got[1] % W == 0)
    assert bool((border & (got[0] == 1)).any()) and not bool((border & (got[0] != 1)).any())
    with pytest.raises(ValueError):
        qi.torch_query_init(h, flat, K, W, nms_free_classes=(C,))


@pytest.mark.parametrize("shape", [qc.SMALL, qc.MID], ids=["24wide", "64wide"])
def test_query_pos_is_the_bev_pos_gather(shape):
    h, flat, K, pos, W = inputs(shape)
    _, top_index, query_pos, _, _ = qi.torch_query_init(h, flat, K, W)
    want = pos.expand(h.shape[0], -1, -1).gather(index=top_index[:, :, None].expand(-1, -1, 2), dim=1)
    assert query_pos.dtype == torch.float32 and torch.equal(query_pos, want)


def test_backward_is_the_ordered_sum():
    h, flat, K, pos, W = inputs(qc.DUPS)
    flat = flat.clone().requires_grad_(True)
    top_index, rows = qi.torch_query_init(h, flat, K, W)[1::3]
    d_rows = torch.randn(rows.shape, generator=torch.Generator().manual_seed(7))
    rows.backward(d_rows)
    want = qc.ordered_backward(top_index, d_rows, h.shape[2] * h.shape[3])
    assert qc.shared_cells(top_index) >= 40
    # indexing's CPU backward accumulates serially in pick order: the same sums, bit for bit, also where three picks share a cell
    assert torch.equal(flat.grad.transpose(1, 2), want)


def test_supported_refuses_what_the_kernels_do_not_cover():
    ok = qi.shape_supported
    assert ok(4, 10, 180, 180, 200, 128, 3, torch.bfloat16) and ok(1, 5, 180, 180, 500, 128, 3, torch.float32)
    assert ok(1, 32, 3, 3, 288, 4, 3, torch.float32)
    assert not ok(4, 10, 180, 180, 200, 128, 1, torch.bfloat16)     # nms_kernel_size != 3
    assert not ok(4, 10, 180, 180, 200, 128, 5, torch.bfloat16)
    assert not ok(4, 10, 180, 180, 513, 128, 3, torch.bfloat16)     # K > 512
    assert not ok(1, 2, 8, 8, 129, 128, 3, torch.bfloat16)          # K > C*H*W
    assert not ok(4, 33, 180, 180, 200, 128, 3, torch.bfloat16)     # C > 32
    assert not ok(4, 10, 2, 180, 200, 128, 3, torch.bfloat16)       # H < 3
    assert not ok(4, 10, 180, 2, 200, 128, 3, torch.bfloat16)       # W < 3
    assert not ok(4, 10, 180, 180, 200, 132, 3, torch.bfloat16)     # 264-byte rows: not whole 16-byte vectors
    assert ok(4, 10, 180, 180, 200, 132, 3, torch.float32)
    assert not ok(4, 10, 180, 180, 200, 130, 3, torch.float32)
    assert not ok(4, 10, 180, 180, 200, 128, 3, torch.float16)      # other dtypes
    assert not ok(4, 10, 180, 180, 200, 128, 3, torch.float64)
    h, flat, K, pos, W = inputs(qc.SMALL)
    assert not qi.supported(h, flat, K)                              # CPU tensors
    with pytest.raises(RuntimeError):
        qi.fused_query_init(h, flat, K, W)
    qc.assert_same(qi.query_init(h, flat, K, W), qi.torch_query_init(h, flat, K, W))   # the dispatcher takes the torch path


def small_head(**kw):
    d = 32
    layer = dict(self_attn_cfg=dict(embed_dims=d, num_heads=4, dropout=0.0), cross_attn_cfg=dict(embed_dims=d, num_heads=4, dropout=0.0),
                 ffn_cfg=dict(embed_dims=d, feedforward_channels=64, num_fcs=2, ffn_drop=0.0),
                 pos_encoding_cfg=dict(input_channel=2, num_pos_feats=d))
    torch.manual_seed(0)
    return BEVFusionHead(num_proposals=20, in_channels=16, hidden_channel=d, num_classes=2, decoder_layer=layer, num_heads=4,
                         grid_size=(24 * 8, 20 * 8, 41), out_size_factor=8, **kw)


def test_head_on_the_cpu_ignores_the_switch(monkeypatch):
    x = torch.randn(2, 16, 24, 20, generator=torch.Generator().manual_seed(3))
    outs = []
    for value in ("0", "1"):
        monkeypatch.setenv("BFHIP_QUERY_INIT", value)
        assert qi.enabled() == (value == "1")
        head = small_head().eval()
        with torch.no_grad():
            outs.append(head([x])[0][0])
    assert sorted(outs[0]) == sorted(outs[1])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_head_nms_free_classes_keyword():
    x = torch.randn(2, 16, 24, 20, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        plain = small_head().eval()([x])[0][0]
        free = small_head(nms_free_classes=(1,)).eval()([x])[0][0]
    assert small_head().nms_free_classes == ()
    assert torch.equal(plain["dense_heatmap"], free["dense_heatmap"])
    h = plain["dense_heatmap"].sigmoid()
    want = qi.torch_query_init(h, torch.zeros(2, 4, 24 * 20), 20, 20, nms_free_classes=(1,))
    assert torch.equal(free["query_labels"], want[0]) and torch.equal(free["query_heatmap_score"], want[3])
    assert not torch.equal(free["query_labels"], plain["query_labels"])
    with pytest.raises(ValueError):
        small_head(nms_free_classes=(2,))
