"""GPU: the fused query initialisation (csrc/query_init.hip through bevfusion_amd/query_init.py) against the torch chain it
replaces on the device, against its own arithmetic (torch_query_init on the CPU) where only the defined order decides, and at
module level with the switch on and off.  Every comparison is bit for bit."""
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import query_init as qi
import query_init_cases as qc
from test_query_init_cpu import small_head

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
IDS = dict(ids=lambda s: "x".join(map(str, s)))


def device_inputs(dev, shape, dtype=F32, channels_last=False, seed=0):
    B, C, H, W, K = shape
    h = qc.distinct_map(shape, seed).to(dev)
    if channels_last:
        h = h.contiguous(memory_format=torch.channels_last)
    flat = qc.features(shape, seed).to(dev, dtype).transpose(1, 2)   # the channels-last view
    return h, flat, K, qc.bev_pos(H, W).to(dev), W


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", qc.SHAPES, **IDS)
def test_parity_with_the_parent_chain(dev, shape, channels_last, dtype):
    h, flat, K, pos, W = device_inputs(dev, shape, dtype, channels_last)
    assert int(qc.positive_peaks(h).min()) >= K
    assert qi.supported(h, flat, K) and flat.stride(1) == 1
    assert h.is_contiguous(memory_format=torch.channels_last) == channels_last or shape[1] == 1
    before = qi.LAUNCHES["fwd"]
    got = qi.query_init(h, flat, K, W)
    assert qi.LAUNCHES["fwd"] == before + 1
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64 and got[4].dtype == dtype
    qc.assert_same(got, qc.parent_chain(h, flat, K, pos), str(shape))


@pytest.fixture(scope="module")
def cpu_orders():
    """torch_query_init on the CPU for every tie case, computed once."""
    out = {}
    for name, (h, K) in qc.tie_cases().items():
        B, C, H, W = h.shape
        feat = torch.randn(B, H * W, qc.CH, generator=torch.Generator().manual_seed(11))
        out[name] = (h, feat, K, qi.torch_query_init(h, feat.transpose(1, 2), K, W))
    return out


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", sorted(qc.tie_cases()))
def test_defined_order(dev, cpu_orders, name, channels_last):
    h, feat, K, want = cpu_orders[name]
    hd = h.to(dev)
    if channels_last:
        hd = hd.contiguous(memory_format=torch.channels_last)
    got = qi.fused_query_init(hd, feat.to(dev).transpose(1, 2), K, h.shape[3])
    qc.assert_same(got, want, name)


@pytest.mark.parametrize("free", [(1,), (0, 2)], ids=["1", "0+2"])
@pytest.mark.parametrize("name", ["distinct", "eighths_small", "short_nan"])
def test_nms_free_classes(dev, name, free):
    if name == "distinct":
        h, K = qc.distinct_map(qc.SMALL), qc.SMALL[4]
    else:
        h, K = qc.tie_cases()[name]
    B, C, H, W = h.shape
    free = tuple(c for c in free if c < C)
    feat = torch.randn(B, H * W, qc.CH, generator=torch.Generator().manual_seed(12))
    want = qi.torch_query_init(h, feat.transpose(1, 2), K, W, nms_free_classes=free)
    got = qi.fused_query_init(h.to(dev), feat.to(dev).transpose(1, 2), K, W, nms_free_classes=free)
    qc.assert_same(got, want, name)
    if name == "distinct":
        assert not torch.equal(want[1], qi.torch_query_init(h, feat.transpose(1, 2), K, W)[1])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_backward_is_the_ordered_f32_sum(dev, dtype):
    h, flat, K, pos, W = device_inputs(dev, qc.DUPS, dtype)
    flat = flat.detach().requires_grad_(True)
    top_index, rows = qi.fused_query_init(h, flat, K, W)[1::3]
    assert qc.shared_cells(top_index.cpu()) >= 40
    d_rows = torch.randn(rows.shape, generator=torch.Generator().manual_seed(7)).to(dev, dtype)
    before = qi.LAUNCHES["bwd"]
    rows.backward(d_rows)
    assert qi.LAUNCHES["bwd"] == before + 1
    assert flat.grad.shape == flat.shape and flat.grad.dtype == dtype
    want = qc.ordered_backward(top_index, d_rows, h.shape[2] * h.shape[3])
    assert torch.equal(flat.grad.transpose(1, 2).cpu(), want)


def test_backward_matches_the_parent_indexing(dev):
    shape = (2, 2, 20, 24, 50)   # two classes: a cell is picked at most twice, and a + b has one value in any order
    h, flat, K, pos, W = device_inputs(dev, shape, F32)
    assert int(qc.positive_peaks(h).min()) >= K
    d_rows = torch.randn(shape[0], K, qc.CH, generator=torch.Generator().manual_seed(8)).to(dev)
    grads = []
    for fn in (lambda f: qi.fused_query_init(h, f, K, W), lambda f: qc.parent_chain(h, f, K, pos)):
        f = flat.detach().requires_grad_(True)
        out = fn(f)
        counts = torch.zeros(shape[0], shape[2] * shape[3], device=dev).scatter_add_(1, out[1], torch.ones_like(out[1], dtype=F32))
        assert int(counts.max()) == 2, "the case must have shared cells, and none picked more than twice"
        out[4].backward(d_rows)
        grads.append(f.grad)
    assert torch.equal(grads[0], grads[1])


def test_two_runs_give_identical_bits(dev):
    h, flat, K, pos, W = device_inputs(dev, qc.MID, BF16, channels_last=True)
    d_rows = torch.randn(h.shape[0], K, qc.CH, generator=torch.Generator().manual_seed(9)).to(dev, BF16)
    runs = []
    for _ in range(2):
        f = flat.detach().requires_grad_(True)
        out = qi.fused_query_init(h, f, K, W)
        out[4].backward(d_rows)
        runs.append(out + (f.grad,))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    for name, (hh, KK) in qc.tie_cases().items():   # plateaus: the append order of the candidates must not show
        feat = torch.randn(hh.shape[0], hh.shape[2] * hh.shape[3], qc.CH, generator=torch.Generator().manual_seed(10)).to(dev)
        a = qi.fused_query_init(hh.to(dev), feat.transpose(1, 2), KK, hh.shape[3])
        b = qi.fused_query_init(hh.to(dev), feat.transpose(1, 2), KK, hh.shape[3])
        qc.assert_same(a, b, name)


def test_no_host_read(dev):
    h, flat, K, pos, W = device_inputs(dev, qc.SMALL, BF16)
    flat = flat.detach().requires_grad_(True)
    d_rows = torch.randn(h.shape[0], K, qc.CH, generator=torch.Generator().manual_seed(9)).to(dev, BF16)
    qi.fused_query_init(h, flat, K, W)   # library load and first launches outside the guarded region
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = qi.fused_query_init(h, flat, K, W)
        out[4].backward(d_rows)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert flat.grad is not None and bool(torch.isfinite(flat.grad.float()).all())


def run_head(dev, monkeypatch, switch, x):
    monkeypatch.setenv("BFHIP_QUERY_INIT", switch)
    head = small_head().to(dev).train()
    kept = {}

    def channels_last(mod, args, out):
        # the shared conv's output as the channels-last tensor the HIP convolution produces in the full model (a small f32
        # layer runs in the library, whose layout follows its input)
        out = out.contiguous(memory_format=torch.channels_last)
        out.retain_grad()
        kept["fusion_feat"] = out
        return out

    head.shared_conv.register_forward_hook(channels_last)
    before = qi.LAUNCHES["fwd"]
    out = head([x])[0][0]
    sum(v.float().sum() for k, v in out.items() if v.is_floating_point() and v.requires_grad).backward()
    return out, head.shared_conv.weight.grad, kept["fusion_feat"].grad, qi.LAUNCHES["fwd"] - before


def test_head_with_the_switch_on_and_off(dev, monkeypatch):
    """The library's f32 weight gradient of these small 3x3 convolutions differs from run to run with the switch off as well (its
    default algorithm adds with atomics), so the comparison runs with torch.backends.cudnn.deterministic, under which two runs of
    the same arm agree bit for bit; the gradient arriving at the shared conv's output is compared too."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    x = torch.randn(2, 16, 24, 20, generator=torch.Generator().manual_seed(3)).to(dev)
    off, g_off, d_off, n_off = run_head(dev, monkeypatch, "0", x)
    on, g_on, d_on, n_on = run_head(dev, monkeypatch, "1", x)
    assert (n_off, n_on) == (0, 1), "the switch must select the fused path"
    assert int(qc.positive_peaks(off["dense_heatmap"].detach().sigmoid()).min()) >= 20
    assert sorted(off) == sorted(on)
    for k in off:
        assert off[k].dtype == on[k].dtype and torch.equal(off[k], on[k]), k
    assert d_off is not None and torch.equal(d_off, d_on)
    assert g_off is not None and torch.equal(g_off, g_on)
