"""GPU: bit-exact parity of every kernel csrc/conv2d.hip and csrc/conv2d_wgrad.hip launch, through the C ABI, on integer-valued
operands (conv_exact_cases.py: why exact, the case table, the checks).  Every output buffer is pre-filled with a sentinel and
carries a guard band, so a kernel that writes a column or row it does not own, or leaves one of its own unwritten, fails too.
The kernels the default knobs cannot reach run in child processes (the knobs are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib

import conv_exact_cases as C
from test_conv2d_exact_cpu import DEFAULT_REACHABLE

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("part", C.PARTS)
@pytest.mark.parametrize("g", C.CASES, ids=C.case_id)
def test_integer_data_is_reproduced_bit_for_bit(dev, g, part):
    """fwd: fp32 and bf16 output (bf16 = the fp32 reference rounded once, bias added before the rounding), stat_partial equal to
    the exact column sums / sums of squares per 128 GEMM rows; dgrad: fp32 and bf16, unreached parity classes zero-filled; wgrad:
    fp32 and bf16 dW.  Each with the case's variation of bias / pitches / statistics and with its complement."""
    C.check_case(dev, g, part)


POINTWISE = [g for g in C.CASES if g[5] == 1 and g[6] == 1 and g[7] == 0]


@pytest.mark.parametrize("mode", ["dense", "pitch", "pair", "odd"])
@pytest.mark.parametrize("addend_stride", [1, 2])
@pytest.mark.parametrize("hw", [(19, 23), (18, 22)], ids=["odd", "even"])
def test_fused_addend_of_the_pointwise_data_gradient(dev, hw, addend_stride, mode):
    assert len(POINTWISE) >= 3
    for g in POINTWISE:    # both tile widths of conv_pw_kernel<NI, false, 1>
        C.check_addend(dev, (g[0],) + hw + g[3:], addend_stride, mode)


def test_batched_weight_transpose_and_dgrad_wt_match_the_per_call_path(dev):
    """One bfhip_conv2d_weight_transpose_batched launch over six segments (1, 9 and 25 taps; channel counts that are no multiples of
    32; bf16 and fp32 sources): every destination equals its permuted source, rounded to bf16 where the source is fp32; and
    bfhip_conv2d_dgrad_wt over the transposed integer weights is bit-identical to bfhip_conv2d_dgrad, guard band included."""
    lib = _lib.load()
    cases = [g for g in C.CASES if g in [(2, 19, 23, 72, 136, 1, 1, 0, 1), (2, 19, 23, 40, 72, 3, 2, 1, 1), (1, 17, 19, 16, 16, 5, 4, 2, 1)]]
    assert sorted(g[5] ** 2 for g in cases) == [1, 9, 25] and all(g[3] % 32 and g[4] % 32 for g in cases)
    rng = np.random.default_rng(17)
    srcs = []
    for i, g in enumerate(cases):      # the cases' integer weights (dgrad_wt below) and random ones of the other source type
        Cout, Cin, taps = g[4], g[3], g[5] ** 2
        w = C.reference(g).w.reshape(Cout, taps, Cin)
        rnd = torch.from_numpy(rng.standard_normal((Cout, taps, Cin)).astype(np.float32))
        srcs.append(w.to(dev).to(torch.float32 if i % 2 == 0 else torch.bfloat16))
        srcs.append(rnd.to(dev).to(torch.bfloat16 if i % 2 == 0 else torch.float32))
    assert lib.bfhip_conv2d_wt_segment_bytes() == 40
    dt = np.dtype([("src", "<u8"), ("dst", "<u8"), ("Cout", "<i4"), ("taps", "<i4"), ("Cin", "<i4"), ("f32", "<i4"), ("blk0", "<i8")])
    dsts, recs, blk = [], [], 0
    for sc in srcs:
        Cout, taps, Cin = sc.shape
        dsts.append(torch.full((sc.numel() + 64,), C.SENT, dtype=torch.bfloat16, device=dev))
        recs.append((sc.data_ptr(), dsts[-1].data_ptr(), Cout, taps, Cin, int(sc.dtype == torch.float32), blk))
        blk += -(-Cin // 32) * -(-Cout // 32) * taps
    table = torch.from_numpy(np.array(recs, dtype=dt).view(np.uint8).copy()).to(dev)
    _lib.call("bfhip_conv2d_weight_transpose_batched", table.data_ptr(), len(recs), blk, _lib.stream_of(table))
    for sc, dst in zip(srcs, dsts):
        assert torch.equal(dst[:sc.numel()], sc.permute(2, 1, 0).contiguous().to(torch.bfloat16).flatten())
        assert bool((dst[sc.numel():] == C.SENT).all())
    for i, g in enumerate(cases):
        N, H, W, Cin, Cout, k, s, p, d = g
        r = C.reference(g)
        for f32 in (0, 1):
            for pitch in (False, True):
                want = C.check_dgrad(dev, g, f32, pitch)
                ldg, ldx = (Cout + 16, Cin + 8) if pitch else (Cout, Cin)
                gb, gp = C._dev_in(r.dy, ldg, 8 if pitch else 0, dev)
                dx = C._dev_out(N * H * W, ldx, want.dtype, dev)
                _lib.call("bfhip_conv2d_dgrad_wt", gp, ldg, dsts[2 * i].data_ptr(), None, 1, dx.data_ptr(), ldx, N, H, W, Cin, Cout,
                          k, k, s, p, d, f32, _lib.stream_of(gb))
                assert torch.equal(dx, want), (C.case_id(g), f32, pitch)


def test_this_process_reaches_every_default_reachable_kernel(dev):
    """What the cases above ran, read through the query with this device's CU count."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    seen = C.variants_of(_lib.load(), C.CASES)
    assert sorted(seen) == sorted(DEFAULT_REACHABLE), "on %d CUs (the table is laid out for 256): missing %s, unexpected %s" % (
        cus, sorted(set(DEFAULT_REACHABLE) - set(seen)), sorted(set(seen) - set(DEFAULT_REACHABLE)))


def test_knob_only_kernels_in_child_processes(dev):
    """Child A: two-stage kernels everywhere (the parity classes included), wide tiles that M does not fill; child B: one stage
    with long K loops, strided plain transposed gather, 1x1 layers on the implicit GEMM.  Each child checks through the query that it
    reached what it is there for, then runs the small cases through the same checks as above.  The first child that does not exit
    0 ends the test: nothing more is started on the device after a failure."""
    torch.cuda.synchronize()
    script = os.path.abspath(C.__file__)
    for name, (env, _) in sorted(C.CHILDREN.items()):
        r = subprocess.run([sys.executable, script, name], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, "child %s exited %d:\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert ("child %s ok" % name) in r.stdout


@pytest.mark.parametrize("Cn", [8, 40])
def test_split_bf16x3_is_bit_exact(dev, Cn):
    """bfhip_split_bf16x3: hi = bf16(v), lo = bf16(v - hi), both layouts, all 8 values of each order word."""
    P = 37
    rng = np.random.default_rng(41 + Cn)
    v = rng.standard_normal((P, Cn)).astype(np.float32) * np.exp2(rng.integers(-20, 20, (P, Cn))).astype(np.float32)
    v[0, :4] = [0.0, -0.0, 1.0, -3.0]
    src = torch.from_numpy(v).to(dev)
    hi = src.to(torch.bfloat16)
    lo = (src - hi.float()).to(torch.bfloat16)
    pair = (hi, lo)
    for m in range(10):    # both layouts with every order word, then each layout alone
        oc, ob = m % 8, 7 - m % 8
        chan = torch.full((P + 1, 3 * Cn), C.SENT, dtype=torch.bfloat16, device=dev) if m != 8 else None
        batch = torch.full((3 * P + 1, Cn), C.SENT, dtype=torch.bfloat16, device=dev) if m != 9 else None
        _lib.call("bfhip_split_bf16x3", src.data_ptr(), P, Cn, _lib.ptr(chan), oc, _lib.ptr(batch), ob, _lib.stream_of(src))
        for k in range(3):
            if chan is not None:
                assert torch.equal(chan[:P, k * Cn:(k + 1) * Cn].view(torch.int16), pair[(oc >> k) & 1].view(torch.int16)), (m, k)
            if batch is not None:
                assert torch.equal(batch[k * P:(k + 1) * P].view(torch.int16), pair[(ob >> k) & 1].view(torch.int16)), (m, k)
        assert chan is None or bool((chan[P] == C.SENT).all())
        assert batch is None or bool((batch[3 * P] == C.SENT).all())
