"""CPU: the case builders of tests/attn_cases.py.  The fp64 reference alone must reproduce every closed form of the selector
cases (no wrong element after bf16 rounding), the numpy restatement of the dropout hash must keep the right share of every
row and every key column, and the size predicate must refuse dropout beyond 2^32 attention weights."""
import math

import numpy as np
import pytest
import torch

import attn_cases as ac
import bevfusion_amd  # noqa: F401
from bevfusion_amd import attention as at

BUILDERS = dict(single=ac.single_case, tie=ac.tie_case, nomatch=ac.nomatch_case)


def test_pairs_cover_every_size_and_both_backward_kernels():
    assert {p[3] for p in ac.PAIRS} == set(ac.KEY_COUNTS) and {p[2] for p in ac.PAIRS} == set(ac.QUERY_COUNTS)
    assert any(p[:2] == (2, 3) for p in ac.PAIRS)
    assert any(p[2] <= 256 for p in ac.PAIRS) and any(p[2] > 256 for p in ac.PAIRS)
    assert 10 <= len(ac.PAIRS) <= 14 and max(ac.KEY_COUNTS) <= 2600


@pytest.mark.parametrize("Lk", ac.KEY_COUNTS)
def test_selected_positions_sit_on_every_seam(Lk):
    pos = ac.single_positions(Lk)
    assert len(pos) == len(set(pos)) == 16 and all(0 <= p < Lk for p in pos)
    want = [p for p in (0, 3, 4, 15, 16, 127, 128, 511, 512, Lk - 1) if p < Lk] + ([Lk // 16 * 16] if Lk % 16 else [])
    assert set(want) <= set(pos)
    pairs = ac.tie_pairs(Lk)
    flat = [x for ab in pairs for x in ab]
    assert len(flat) == len(set(flat)) and all(0 <= a < b < Lk for a, b in pairs)
    last = (Lk - 1) // 512
    assert any(a // 4 == b // 4 for a, b in pairs)                                             # one lane group
    assert any(a // 4 + 1 == b // 4 and a // 16 == b // 16 for a, b in pairs)                  # adjacent lane groups
    assert any(a // 16 + 1 == b // 16 and a // 128 == b // 128 for a, b in pairs)              # adjacent tiles
    assert Lk <= 128 or any(a // 128 + 1 == b // 128 and a // 512 == b // 512 for a, b in pairs)  # adjacent waves
    assert last == 0 or any(a // 512 + 1 == b // 512 and a + 1 == b for a, b in pairs)         # adjacent chunks
    assert any(a // 512 == 0 and b // 512 == last and b - a > 1 or last == 1 for a, b in pairs)  # first and last chunk
    assert any(b == Lk - 1 for a, b in pairs)                                                  # the last key


@pytest.mark.parametrize("Lq", ac.QUERY_COUNTS)
def test_marked_queries_carry_a_code(Lq):
    """Every query carries a code, so queries 0, 15, 16, 255, 256 and Lq - 1 do; the codes differ from tile to tile."""
    code = ac.query_code(Lq, 0)
    assert code.shape == (Lq,) and code.min() >= 0 and code.max() < 16
    if Lq > 16:
        assert code[0] != code[16]
    q = ac.single_case(1, 1, Lq, 70)["q"].double()
    for i in {0, 15, 16, 255, 256, Lq - 1}:
        if i < Lq:
            assert torch.equal(q[0, i].abs(), torch.full((16,), 4.0, dtype=torch.float64))


def test_reference_is_scaled_dot_product_attention():
    """Without its rounding points the reference equals torch's own fp64 softmax attention and autograd."""
    c = ac.gaussian_case(2, 3, 17, 70, seed=5, std=1.0)
    ref = ac.reference(c["q"], c["k"], c["v"], c["do"], 3, rounded=False)
    q, k, v = [c[n].double().requires_grad_(True) for n in "qkv"]
    hq, hk, hv = [t.view(2, -1, 3, 16).transpose(1, 2) for t in (q, k, v)]
    o = ((hq @ hk.transpose(-1, -2) / 4).softmax(-1) @ hv).transpose(1, 2).reshape(2, 17, 48)
    o.backward(c["do"].double())
    for got, want in ((ref["o"], o.detach()), (ref["dq"], q.grad), (ref["dk"], k.grad), (ref["dv"], v.grad)):
        assert float((got - want).abs().max()) < 1e-12


def test_reference_applies_the_keep_mask():
    c = ac.gaussian_case(1, 2, 5, 70, seed=6)
    keep = ac.keep_mask(1, 2, 5, 70, 0.5, 9)
    ref = ac.reference(c["q"], c["k"], c["v"], c["do"], 2, keep=keep, p=0.5, rounded=False)
    plain = ac.reference(c["q"], c["k"], c["v"], c["do"], 2, rounded=False)
    hv = c["v"].double().view(1, 70, 2, 16).transpose(1, 2)
    want = (plain["p"] * torch.from_numpy(keep) * 2) @ hv
    assert float((ref["o"] - want.transpose(1, 2).reshape(1, 5, 32)).abs().max()) < 1e-14


@pytest.mark.parametrize("B,H,Lq,Lk", ac.PAIRS)
@pytest.mark.parametrize("kind,amp", [("single", 4), ("tie", 4), ("nomatch", 4), ("single", 8), ("tie", 8)])
def test_reference_reproduces_the_closed_forms(kind, amp, B, H, Lq, Lk):
    c = BUILDERS[kind](B, H, Lq, Lk) if kind == "nomatch" else BUILDERS[kind](B, H, Lq, Lk, amp=amp)
    for n in "qkv":
        x = c[n].double()
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= 8  # small integers: exact in bf16
    x = c["do"].double()
    assert torch.equal(x, x.round()) and float(x.abs().max()) <= 8
    ref = ac.reference(c["q"], c["k"], c["v"], c["do"], H)
    for name, want in c["expect"].items():
        assert ac.exact_mismatch(ref[name], want) == (0, 0.0), (kind, name)
    if kind == "single":  # the residue of the unselected keys is far below the bound it is held to
        assert float(ref["dq"].abs().max()) < 1e-22 and float(ref["dk"].abs().max()) < 1e-22
        assert float(c["expect"]["dv"].abs().max()) > 0
    if kind == "tie":
        assert float(c["expect"]["dk"].abs().max()) > 0
        assert float((ref["p"].max(-1).values - 0.5).abs().max()) < 1e-12


@pytest.mark.parametrize("B,H,Lq,Lk", ac.PAIRS)
def test_logit_64_cases_never_cancel(B, H, Lq, Lk):
    """At logit 64 no sum whose closed form is zero may pass through a partial sum that is a power of two (the matrix core
    would leave an fp32 ulp behind): dO has one sign per channel and no zero, every dV and dK entry of a selected key is
    non-zero unless all its terms are, and |dO.(V_a - V_b)| is no power of two.  At logit 256 the data is free."""
    for build in (ac.single_case, ac.tie_case):
        c = build(B, H, Lq, Lk)
        do = c["do"].double()
        assert float(do.abs().min()) >= 1 and bool(((do > 0).all(1) | (do < 0).all(1)).all())
        free = build(B, H, Lq, Lk, amp=8)["do"].double()
        assert Lq < 16 or not bool(((free > 0).all(1) | (free < 0).all(1)).all())
    c = ac.tie_case(B, H, Lq, Lk)
    ref = ac.reference(c["q"], c["k"], c["v"], c["do"], H)
    hv, hdo = [t.double().view(B, -1, H, 16).transpose(1, 2) for t in (c["v"], c["do"])]
    sel = ref["p"] > 0.25                                        # the two selected keys of every query
    assert bool((sel.sum(-1) == 2).all())
    da = hdo @ hv.transpose(-1, -2)                              # dO.V per (query, key)
    first = sel & (sel.cumsum(-1) == 1)
    x = (da * first).sum(-1) - (da * (sel & ~first)).sum(-1)     # dO.(V_a - V_b) per query
    assert bool((x >= 0).all()) and float(x.max()) <= 128
    assert not any(ac._is_pow2(val) for val in x.flatten().tolist())
    picked = sel.any(2)                                          # [B, H, Lk]: keys that some query selects
    dk, dv = [c["expect"][n].view(B, -1, H, 16).transpose(1, 2) for n in ("dk", "dv")]
    assert bool((dv[picked] != 0).all())                         # sums of dO / 2 of one sign
    xsum = (x[..., None] * sel).sum(2)                           # [B, H, Lk]: the sum of x over the queries of a key
    assert bool(((dk != 0).all(-1) == (xsum > 0))[picked].all()) and bool(((dk == 0).all(-1) == (xsum == 0))[picked].all())


def test_exact_comparison_sees_one_ulp_and_a_residue():
    want = torch.tensor([1.0, 0.0, 3.0], dtype=torch.float64)
    assert ac.exact_mismatch(torch.tensor([1.0, 1e-24, 3.0]).to(torch.bfloat16), want) == (0, 0.0)
    assert ac.exact_mismatch(torch.tensor([1.0078125, 0.0, 3.0]).to(torch.bfloat16), want)[0] == 1
    assert ac.exact_mismatch(torch.tensor([1.0, 1e-19, 3.0]).to(torch.bfloat16), want)[0] == 1
    assert ac.exact_mismatch(torch.tensor([1.0, float("nan"), float("nan")]).to(torch.bfloat16), want)[0] == 2


@pytest.mark.parametrize("Lk", ac.KEY_COUNTS + (2048,))
def test_uniform_weight_is_far_from_a_bf16_rounding_boundary(Lk):
    """bf16(exp(-lse)) must not depend on the last bits of the hardware's log and exp (relative error ~1e-6): 1 / Lk lies at
    least 1e-4 of its value away from the nearest boundary between two bf16 numbers -- except 1 / 513, which sits 3.8e-6 from
    the boundary between 255/256 x 2^-9 and 2^-9: there both neighbours are candidates."""
    ws = ac.uniform_weights(Lk)
    if Lk == 513:
        assert ac.weight_rounding_margin(Lk) < 1e-5 and ws == (2.0 ** -9, 255 * 2.0 ** -17)
    else:
        assert ac.weight_rounding_margin(Lk) > ac.MARGIN and ws == (float(ac.bf16_round(1.0 / Lk)),)
    for w in ws:
        assert float(ac.bf16_round(w)) == w and abs(w * Lk - 1) < 2.0 ** -8
    if Lk & (Lk - 1) == 0:
        assert ws == (1.0 / Lk,)
    assert len(ac.nomatch_case(1, 1, 1, Lk)["alt"]) == len(ws) - 1


def test_nomatch_is_the_exact_mean_at_a_power_of_two():
    c = ac.nomatch_case(1, 2, 16, 512)
    mean = c["v"].double().mean(1, keepdim=True).expand(1, 16, 32)
    assert torch.equal(ac.bf16_round(c["expect"]["o"]), ac.bf16_round(mean))


# ------------------------------------------------------------------------------------------------ the hash in numpy
def test_eff_seed_wraps_in_64_bits():
    assert ac.eff_seed(7, 0) == 7
    assert ac.eff_seed(7, 3) == 7 + 3 * 0xD1B54A32D192ED03 - 2 * (1 << 64)
    assert ac.eff_seed((1 << 64) - 1, 1) == 0xD1B54A32D192ED03 - 1
    assert int(ac.thresh24(0.5)) == 1 << 23 and int(ac.thresh24(0.1)) == int(np.float32(0.1) * np.float32(2.0) ** 24) == 1677721


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", [1234567, 0x9E3779B97F4A7C15])
def test_keep_rate_per_row_and_per_key_column(p, seed):
    """Keep counts are binomial(n, 1 - p): every row (n = Lk) and every key column (n = B*H*Lq) within 5 sigma, the whole
    mask as well."""
    B, H, Lq, Lk = 1, 2, 256, 2048
    keep = ac.keep_mask(B, H, Lq, Lk, p, seed)
    t = int(ac.thresh24(p))
    rate = 1.0 - t / 2.0 ** 24
    for name, counts, n in (("row", keep.sum(-1).ravel(), Lk), ("column", keep.sum((0, 1, 2)), B * H * Lq), ("all", keep.sum(), keep.size)):
        dev = np.abs(np.asarray(counts, np.float64) - n * rate).max() / math.sqrt(n * rate * (1 - rate))
        print("p", p, name, "max deviation in sigma:", dev)
        assert dev < 5.0, (name, dev)


def test_seeds_and_counters_change_the_mask():
    a = ac.keep_mask(1, 2, 16, 512, 0.5, 42)
    for other in (ac.keep_mask(1, 2, 16, 512, 0.5, 43), ac.keep_mask(1, 2, 16, 512, 0.5, 42 + (1 << 32)),
                  ac.keep_mask(1, 2, 16, 512, 0.5, 42, counter=1)):
        share = float((a != other).mean())
        assert 0.45 < share < 0.55, share  # independent masks differ in half their elements (16 384 draws: 5 sigma = 0.02)
    assert np.array_equal(ac.keep_mask(1, 2, 16, 512, 0.5, 42, counter=3), ac.keep_mask(1, 2, 16, 512, 0.5, ac.eff_seed(42, 3)))
    assert ac.keep_mask(1, 1, 4, 70, 0.0, 1).all()


# ------------------------------------------------------------------------------------------------ the 2^32 rule
class _Shape:
    """What the predicates read of a tensor: no storage behind it."""

    def __init__(self, *shape, dtype=torch.bfloat16, is_cuda=True):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, is_cuda

    def dim(self):
        return len(self.shape)


def test_predicate_refuses_dropout_beyond_2_to_32_weights():
    """The kernels hash a 32-bit element index: with dropout, B*H*Lq*Lk <= 2^32 or the call goes to the library path."""
    H = 8
    q, k = _Shape(2, 256, 128), _Shape(2, 1 << 20, 128)  # 2 * 8 * 256 * 2^20 = 2^32: the last index is 2^32 - 1
    assert at.supported(q, k, k, H) and at.supported(q, k, k, H, 0.1)
    k1 = _Shape(2, (1 << 20) + 1, 128)
    assert at.supported(q, k1, k1, H) and at.supported(q, k1, k1, H, 0.0) and not at.supported(q, k1, k1, H, 0.1)
    assert at._eligible(q, k1, k1, H) and not at._eligible(q, k1, k1, H, 0.5)
    q3 = _Shape(3, 256, 128)
    k3 = _Shape(3, 1 << 20, 128)
    assert not at.supported(q3, k3, k3, H, 0.1) and at.supported(q3, k3, k3, H)
    # the decoder's own shape is nowhere near the limit
    assert at.supported(_Shape(4, 200, 128), _Shape(4, 32400, 128), _Shape(4, 32400, 128), H, 0.1)
