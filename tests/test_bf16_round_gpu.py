"""The fp32 -> bf16 rounding rule of csrc/bf16.h (bf16_rne), stated on its own: round to nearest, ties to even, overflow to
inf, and a NaN stays a NaN -- also one whose payload sits in the low 16 bits only, which the bare add-and-shift would turn
into inf.

Reached through bfhip_split_bf16x3 (conv2d._split3): its "hi" block is bf16_rne of the input and nothing else
(split_bf16x3_kernel: hi[j] = bf16_rne(v[j])).  Every non-NaN element must equal torch's own CPU conversion bit for bit.
The input is the smallest the entry point takes in C (8 channels), 4 pixels: 32 hand-written bit patterns."""
import numpy as np
import pytest
import torch

import bevfusion_amd  # noqa: F401
from bevfusion_amd import conv2d

# (fp32 bits, bf16 bits the rule gives; None = any NaN)
CASES = [
    # exact ties: above an even mantissa the tie goes down, above an odd one up; with the value just below and just above
    (0x3f807fff, 0x3f80), (0x3f808000, 0x3f80), (0x3f808001, 0x3f81),
    (0x3f817fff, 0x3f81), (0x3f818000, 0x3f82), (0x3f818001, 0x3f82),
    (0xbf807fff, 0xbf80), (0xbf808000, 0xbf80), (0xbf808001, 0xbf81),
    (0xbf817fff, 0xbf81), (0xbf818000, 0xbf82), (0xbf818001, 0xbf82),
    # the largest finite fp32 rounds to inf; inf and zero keep their sign
    (0x7f7fffff, 0x7f80), (0xff7fffff, 0xff80), (0x7f800000, 0x7f80), (0xff800000, 0xff80), (0x00000000, 0x0000), (0x80000000, 0x8000),
    # denormals: the smallest, a tie above 0 (even), a tie above an odd mantissa, the largest (rounds up to the smallest normal)
    (0x00000001, 0x0000), (0x00008000, 0x0000), (0x00018000, 0x0002), (0x007fffff, 0x0080),
    # NaN: payload in the low 16 bits only (upper half 0x7f80 / 0xff80), the default quiet NaN, all mantissa bits set
    (0x7f800001, None), (0x7f808000, None), (0xff800001, None), (0x7fc00000, None), (0x7fffffff, None),
    # ordinary values
    (0x3f800000, 0x3f80), (0xc0200000, 0xc020), (0x40490fdb, 0x4049), (0x3a83126f, 0x3a83), (0x477fe000, 0x4780),
]


def _input():
    bits = np.array([b for b, _ in CASES], np.uint32)
    return torch.from_numpy(bits.view(np.float32).reshape(4, 8).copy())


def test_cases_agree_with_torch_cpu():
    """The hand-written expectations are what torch's CPU conversion gives (the reference of the GPU comparison below)."""
    x = _input()
    got = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).ravel()
    for (b, want), g, v in zip(CASES, got, x.ravel()):
        if want is None:
            assert torch.isnan(v) and (g & 0x7f80) == 0x7f80 and (g & 0x007f) != 0, hex(b)
        else:
            assert g == want, (hex(b), hex(g), hex(want))


@pytest.mark.gpu
def test_hi_block_is_round_to_nearest_even(dev):
    x = _input()
    P, C = x.shape
    chan, _ = conv2d._split3(x.to(dev), P, C, chan_order=0)  # order word 0: all three blocks hold hi
    torch.cuda.synchronize()
    hi = chan[:, :C].cpu()
    nan = torch.isnan(x)
    assert int(nan.sum()) == 5
    assert torch.equal(hi.view(torch.int16)[~nan], x.to(torch.bfloat16).view(torch.int16)[~nan])
    assert bool(torch.isnan(hi.float()[nan]).all())
