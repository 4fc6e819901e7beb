"""GPU: split-key cross attention (csrc/attn.hip) against expectations that one wrong key, query or mask bit breaks.

tests/test_attn_gpu.py and tests/test_attn_wide_gpu.py bound the error by 2e-2 of the tensor maximum, under which a single
key among thousands is invisible in O and dQ, and they read the keep mask back from the kernels themselves.  Here:
selector cases with closed-form outputs and gradients (tests/attn_cases.py) are compared for equality, `lse` is compared with
fp64 to a quarter of the smallest softmax weight, the keep mask is compared with a numpy restatement of the hash, the mask
each kernel applies is read out of O and dV bit for bit, and the device step counter is set to a non-zero value."""
import numpy as np
import pytest
import torch

import attn_cases as ac
import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib
from bevfusion_amd import attention as at

pytestmark = pytest.mark.gpu

BUILDERS = dict(single=ac.single_case, tie=ac.tie_case, nomatch=ac.nomatch_case)


def run(dev, c, p=0.0, seed=0):
    """cross_attention forward + backward on a case: O, dQ, dK, dV as bf16 tensors."""
    q, k, v = [c[n].to(dev).requires_grad_(True) for n in "qkv"]
    o = at.cross_attention(q, k, v, c["H"], p, seed)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), c["do"].to(dev))
    return dict(o=o.detach(), dq=dq, dk=dk, dv=dv)


def mismatches(got, expect, tiny=ac.TINY):
    res = {n: ac.exact_mismatch(got[n], want, tiny) for n, want in expect.items()}
    print("wrong elements, largest difference:", res)
    return {n: r for n, r in res.items() if r[0]}


# ---------------------------------------------------------------------------------------- 1. selector cases
@pytest.mark.parametrize("B,H,Lq,Lk", ac.PAIRS)
@pytest.mark.parametrize("kind", ["single", "tie"])
def test_selected_keys_come_out_exactly(dev, kind, B, H, Lq, Lk):
    """Logit 64 on a match.  One key per code: O = V[sel], dV[sel] = sum of dO, dQ = dK = 0.  Two keys per code across every
    seam: weights 1/2, O = (V_a + V_b) / 2, dS = +-dO.(V_a - V_b) / 16, dK and dV from those.  Equality; below 1e-20 where the
    closed form is zero.  dQ of the ties has the next test to itself.
    The data keeps sums over queries from cancelling (attn_cases: NO CANCELLATION): with freely signed dO and before the
    backward dropped negligible weights, the exp(-64) terms left 2^-21 and 2^-22 in one or two dV elements of three single-key
    cases, where the sum of dO over the queries of a key is zero -- the matrix core's flooring adder."""
    c = BUILDERS[kind](B, H, Lq, Lk)
    expect = {n: w for n, w in c["expect"].items() if (kind, n) != ("tie", "dq")}
    assert not mismatches(run(dev, c), expect)


@pytest.mark.parametrize("B,H,Lq,Lk", ac.PAIRS)
def test_tied_keys_leave_no_query_gradient(dev, B, H, Lq, Lk):
    """Logit 64, two keys per code: dQ = dS_a K_a + dS_b K_b = x/4 h - x/4 h = 0, held to 1e-20 like every other zero.
    This is the test that found the negligible-weight rule of attn_bwd_kernel (kNegligible): without it between 8 and 2 228
    elements of dQ held -2^-20 .. -2^-22 in all twelve cases.  v_mfma_f32_16x16x16_bf16 aligns its terms to the largest one,
    keeps one bit below the fp32 result and floors, so the dS K terms of the OTHER codes' keys (about -1e-26, from weights of
    exp(-64)) took 2^-24 of x/4 off the sum before x/4 h - x/4 h cancelled (one instruction alone: accumulator -2^-90,
    products 4 and -4 -> -2^-22).  The backward now counts weights below e^-40 as zero."""
    c = ac.tie_case(B, H, Lq, Lk)
    assert not mismatches(run(dev, c), dict(dq=c["expect"]["dq"]))


def test_backward_drops_weights_below_e_minus_40_only(dev):
    """One key per code at logit 36 (codes x 3): an unselected key weighs e^-36, above the cut, and its dV row is
    bf16(e^-36) x the sum of dO over all queries (one sign per channel: never zero).  At logit 64 the same rows, and dQ, are
    exact zeros."""
    kept = ac.single_case(1, 2, 16, 70, amp=3)
    dv = run(dev, kept)["dv"].double().cpu()
    unselected = kept["k"].double().abs().sum(-1) == 0                                 # [B, Lk]
    want = float(ac.bf16_round(np.exp(-36.0))) * kept["do"].double().sum(1, keepdim=True)  # [B, 1, E]
    rel = ((dv - want).abs() / want.abs())[unselected]
    print("dV of unselected keys at logit 36: max relative error", float(rel.max()))
    assert float(rel.max()) < 2.0 ** -7  # the weight may round to either bf16 neighbour (2^-8), the result is rounded once (2^-9)
    cut = ac.single_case(1, 2, 16, 70)
    got = run(dev, cut)
    assert bool((got["dv"][(cut["k"].double().abs().sum(-1) == 0).to(dev)] == 0).all()) and bool((got["dq"] == 0).all())


@pytest.mark.parametrize("B,H,Lq,Lk", ac.PAIRS)
@pytest.mark.parametrize("kind", ["single", "tie"])
def test_selected_keys_at_logit_256_leave_exact_zeros(dev, kind, B, H, Lq, Lk):
    """The same cases with the codes x 8: exp(-256) underflows, the unselected weights are exactly zero, dO and V_a - V_b are
    free in sign.  Equality, and an exact zero wherever the closed form is zero -- dQ of the ties included, whose two halves
    come from different lane groups, tiles, waves and chunks."""
    c = BUILDERS[kind](B, H, Lq, Lk, amp=8)
    assert not mismatches(run(dev, c), c["expect"], tiny=0.0)


@pytest.mark.parametrize("B,H,Lq,Lk", ac.PAIRS)
def test_unmatched_queries_average_the_valid_keys(dev, B, H, Lq, Lk):
    """Q = 0: O = bf16(w sum V) with w = bf16(1 / Lk) -- the weights are rounded to bf16 before the second MFMA, so this is the
    mean of V exactly where Lk is a power of two and one weight rounding away from it elsewhere.  A padded key that leaks into
    the sum of weights moves w.  dV = bf16(w sum dO) and dK = 0 likewise.
    Lk = 513 alone is soft: 1 / 513 lies 3.8e-6 (relative) from the boundary between the bf16 numbers 255/256 x 2^-9 and 2^-9,
    inside the error of the hardware's log and exp, so either weight is accepted there -- for the whole tensor at once, which
    holds every element within one bf16 ulp of the expectation."""
    c = ac.nomatch_case(B, H, Lq, Lk)
    got = run(dev, c)
    bad = mismatches(got, c["expect"])
    for alt in c["alt"]:
        if bad:
            print("second candidate weight:")
            bad = mismatches(got, alt)
    assert not bad


# ---------------------------------------------------------------------------------------- 2. lse
def _fwd_direct(dev, c, p=0.0, seed=0, seed_dev=None):
    q, k, v = [c[n].to(dev) for n in "qkv"]
    (B, Lq, E), Lk, H = q.shape, k.shape[1], c["H"]
    o = torch.empty_like(q)
    lse = torch.empty(B * H, Lq, dtype=torch.float32, device=dev)
    ws = torch.empty(max(_lib.call_size("bfhip_attn_workspace_bytes", B, H, Lq, Lk), 256), dtype=torch.uint8, device=dev)
    _lib.call("bfhip_attn_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), B, H, Lq, Lk, ac.SCALE, p, seed, seed_dev,
              o.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_of(q))
    return o, lse.view(B, H, Lq)


@pytest.mark.parametrize("B,H,Lq,Lk", ac.PAIRS)
def test_lse_matches_fp64(dev, B, H, Lq, Lk):
    """log-sum-exp of the scaled scores against torch.logsumexp in fp64 on the same bf16 inputs (Gaussian x 0.5).  Tolerance:
    a quarter of the smallest softmax weight of the case -- dropping or doubling ANY one key moves lse by about its weight.
    Measured on an MI355X: max |err| 2.2e-7 (Lk = 70) to 1.1e-6 (Lk = 2049) over the twelve cases, the fp32 noise of a value
    near ln Lk + 0.03; tolerances 2.4e-5 to 2.1e-3, so 21x to 9 700x headroom."""
    c = ac.gaussian_case(B, H, Lq, Lk, seed=Lq * 4099 + Lk)
    ref = ac.reference(c["q"], c["k"], c["v"], c["do"], H, rounded=False)
    tol = float(ref["p"].min()) / 4
    _, lse = _fwd_direct(dev, c)
    err = float((lse.cpu().double() - ref["lse"]).abs().max())
    print("lse max |err| %.3e, tolerance %.3e (smallest weight / 4), headroom %.0fx" % (err, tol, tol / max(err, 1e-30)))
    assert err < tol


def test_lse_of_the_selector_cases(dev):
    """64 with one selected key, 64 + ln 2 with two (fp32 rounding of the sum only), ln Lk with none."""
    for kind, want in (("single", 64.0), ("tie", 64.0 + np.log(2.0)), ("nomatch", np.log(1100.0))):
        _, lse = _fwd_direct(dev, BUILDERS[kind](2, 3, 257, 1100))
        err = float((lse.double() - want).abs().max())
        print(kind, "lse max |err|", err)
        assert err <= (0.0 if kind == "single" else 2.0 ** -17 if kind == "tie" else 2e-6)


# ---------------------------------------------------------------------------------------- 3. the mask against numpy
@pytest.mark.parametrize("seed", [1234567, 0xD1B54A32D192ED03, (5 << 32) | 7])
@pytest.mark.parametrize("B,H,Lq,Lk,p", [(2, 3, 17, 513, 0.1), (1, 2, 257, 1100, 0.5), (1, 1, 512, 70, 0.1)])
def test_dropout_mask_equals_the_numpy_hash(dev, B, H, Lq, Lk, p, seed):
    got = at.dropout_mask(B, H, Lq, Lk, p, seed, dev).cpu().numpy()
    want = ac.keep_mask(B, H, Lq, Lk, p, seed)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not np.array_equal(want, ac.keep_mask(B, H, Lq, Lk, p, seed & 0xFFFFFFFF)) or seed >> 32 == 0


# ---------------------------------------------------------------------------------------- 4. the mask each kernel applies
LK4, P4, SEED4 = 2048, 0.5, (3 << 32) | 99


def _uniform_case(B, H, Lq, v=None, do=None):
    """Q = 0 over 2 048 keys, dropout 0.5: every kept weight is 2^-11 x 2 = 2^-10 exactly (bf16)."""
    E = H * 16
    z = torch.zeros(B, Lq, E, dtype=torch.bfloat16)
    k = torch.zeros(B, LK4, E, dtype=torch.bfloat16)
    v = k if v is None else v.to(torch.bfloat16).repeat(1, 1, H).expand(B, LK4, E).contiguous()
    do = z if do is None else do.to(torch.bfloat16).repeat(1, 1, H).expand(B, Lq, E).contiguous()
    return dict(H=H, q=z, k=k, v=v, do=do)


@pytest.fixture(scope="module")
def keep4():
    cache = {}

    def get(B, H, Lq):
        if (B, H, Lq) not in cache:
            cache[B, H, Lq] = ac.keep_mask(B, H, Lq, LK4, P4, SEED4)
        return cache[B, H, Lq]
    return get


@pytest.mark.parametrize("Lq", [200, 257])
@pytest.mark.parametrize("subset", ["wave", "lane"])
def test_forward_applies_the_numpy_mask(dev, keep4, Lq, subset):
    """V[key, c] = (key in subset c): O[q, c] x 2^10 counts the kept keys of query q in subset c (at most 128: exact in bf16).
    Subsets: the 16 runs of 128 keys (one wave of one chunk each), and the 16 residues key mod 16 (one tile row each)."""
    B, H = 2, 3
    key = torch.arange(LK4)
    member = (key // 128 if subset == "wave" else key % 16)[:, None] == torch.arange(16)[None, :]  # [Lk, 16]
    c = _uniform_case(B, H, Lq, v=member[None].float())
    q, k, v = [c[n].to(dev) for n in "qkv"]
    o = at.cross_attention(q, k, v, H, P4, SEED4)
    got = (o.float().cpu() * 1024).view(B, Lq, H, 16).transpose(1, 2).numpy()  # [B, H, Lq, 16]
    keep = keep4(B, H, Lq)
    want = np.einsum("bhqk,kc->bhqc", keep.astype(np.float32), member.float().numpy())
    wrong = np.argwhere(got != want)
    print("queries with a wrong count:", len(wrong), wrong[:4].tolist())
    assert len(wrong) == 0


@pytest.mark.parametrize("Lq,t", [(200, 0), (200, 12), (512, 0), (512, 15), (512, 16), (512, 31), (257, 16)])
def test_backward_applies_the_numpy_mask(dev, keep4, Lq, t):
    """dO[q, c] = (q == 16 t + c): dV[key, c] x 2^10 = keep[16 t + c, key], the whole mask of query tile t as the backward
    kernel applied it (Lq = 200: attn_bwd_kernel<true, 16>; 257 and 512: <true, 32>; t = 16 at Lq = 257 is the one-query tile)."""
    B, H = 1, 2
    qi = torch.arange(Lq)
    do = (qi[:, None] == 16 * t + torch.arange(16)[None, :]).float()  # [Lq, 16]
    assert do.sum() == min(16, Lq - 16 * t)
    c = _uniform_case(B, H, Lq, do=do[None])
    got = run(dev, c, P4, SEED4)["dv"]
    got = (got.float().cpu() * 1024).view(B, LK4, H, 16).permute(0, 2, 3, 1).numpy()  # [B, H, c, key]
    keep = keep4(B, H, Lq)
    want = np.zeros((B, H, 16, LK4), np.float32)
    n = min(16, Lq - 16 * t)
    want[:, :, :n] = keep[:, :, 16 * t:16 * t + n]
    wrong = np.argwhere(got != want)
    print("wrong mask elements:", len(wrong), wrong[:4].tolist())
    assert len(wrong) == 0


# ---------------------------------------------------------------------------------------- 5. the step counter
def _all_outputs(dev, c, p, seed):
    r = run(dev, c, p, seed)
    return [r[n] for n in ("o", "dq", "dk", "dv")]


def test_step_counter_is_mixed_into_the_seed(dev):
    """Counter 3 with host seed s == counter 0 with host seed s + 3 x 0xD1B54A32D192ED03 (mod 2^64): mask, output and all three
    gradients bit for bit; with p = 0 the counter changes nothing."""
    B, H, Lq, Lk, p, seed = 2, 3, 37, 700, 0.5, 0xF00000000000BEEF  # seed + 3 x step wraps past 2^64
    c = ac.gaussian_case(B, H, Lq, Lk, seed=11, std=1.0)
    other = ac.eff_seed(seed, 3)
    assert other == (seed + 3 * 0xD1B54A32D192ED03) % (1 << 64) and seed + 3 * 0xD1B54A32D192ED03 > (1 << 64)
    counter = at.step_counter(dev)
    assert int(counter) == 0
    base = _all_outputs(dev, c, p, seed)
    moved = _all_outputs(dev, c, p, other)
    plain = _all_outputs(dev, c, 0.0, seed)
    mask0 = at.dropout_mask(B, H, Lq, Lk, p, seed, dev).cpu().numpy()
    try:
        counter.fill_(3)
        mask3 = at.dropout_mask(B, H, Lq, Lk, p, seed, dev).cpu().numpy()
        stepped = _all_outputs(dev, c, p, seed)
        plain3 = _all_outputs(dev, c, 0.0, seed)
    finally:
        counter.zero_()
    assert not np.array_equal(mask3, mask0)
    assert np.array_equal(mask0, ac.keep_mask(B, H, Lq, Lk, p, seed))
    assert np.array_equal(mask3, ac.keep_mask(B, H, Lq, Lk, p, seed, counter=3))
    for name, a, b, z in zip(("o", "dq", "dk", "dv"), stepped, moved, base):
        assert torch.equal(a, b), name
        assert not torch.equal(a, z), name
    for name, a, b in zip(("o", "dq", "dk", "dv"), plain3, plain):
        assert torch.equal(a, b), name
    assert int(counter) == 0


# ---------------------------------------------------------------------------------------- 6. the 32-bit element index
def test_entry_points_refuse_dropout_beyond_2_to_32_weights(dev):
    """B*H*Lq*Lk > 2^32 with dropout: BFHIP_E_INVALID from all three entry points, before any launch (the buffers are tiny).
    Without dropout, and at exactly 2^32, the size check passes: the call goes on to the workspace check and stops there."""
    lib = _lib.load()
    t = torch.zeros(64, dtype=torch.bfloat16, device=dev)
    f = torch.zeros(64, dtype=torch.float32, device=dev)
    m = torch.zeros(64, dtype=torch.uint8, device=dev)
    s = _lib.stream_of(t)
    B, H, Lq = 2, 8, 512
    at_limit, beyond = 1 << 19, (1 << 19) + 1  # 2 * 8 * 512 * 2^19 = 2^32

    def fwd(Lk, p):
        return lib.bfhip_attn_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), B, H, Lq, Lk, 0.25, p, 1, None, t.data_ptr(),
                                  f.data_ptr(), m.data_ptr(), m.numel(), s)

    def bwd(Lk, p):
        return lib.bfhip_attn_bwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), f.data_ptr(), B, H, Lq,
                                  Lk, 0.25, p, 1, None, t.data_ptr(), t.data_ptr(), t.data_ptr(), m.data_ptr(), m.numel(), s)

    def mask(Lk, p):  # no mask buffer: a call that passes the size check stops at the null pointer
        return lib.bfhip_attn_dropout_mask(B, H, Lq, Lk, p, 1, None, None, s)

    for fn in (fwd, bwd, mask):
        rc = fn(beyond, 0.1)
        msg = lib.bfhip_last_error().decode()
        assert rc == -1 and "2^32" in msg and "32-bit" in msg, (fn.__name__, rc, msg)
        for Lk, p in ((beyond, 0.0), (at_limit, 0.1)):
            rc = fn(Lk, p)
            msg = lib.bfhip_last_error().decode()
            assert rc != 0 and "2^32" not in msg, (fn.__name__, Lk, p, rc, msg)
            assert ("workspace" in msg) == (fn is not mask), (fn.__name__, msg)
    torch.cuda.synchronize()
    # the Python predicate says the same, from shapes alone
    q = t[:1].expand(B, Lq, 128)
    k = t[:1].expand(B, beyond, 128)
    assert at.supported_wide(q, k, k, H) and at.supported_wide(q, k, k, H, 0.0) and not at.supported_wide(q, k, k, H, 0.1)
