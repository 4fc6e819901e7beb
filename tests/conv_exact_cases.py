"""Shared case table of the bit-exact convolution tests (test_conv2d_exact_cpu.py, test_conv2d_exact_gpu.py and the child
processes the latter starts); a helper module, not collected by pytest.

Why exact: with integer-valued operands (x in [-3, 3], w in [-2, 2], dy in [-2, 2], bias in [-4, 4]) every product and every
partial sum of a convolution is an integer far below 2^24, so it is exact in fp32 whatever the summation order, the tile shape,
the K split or the number of LDS stages.  An fp32 output must therefore EQUAL the CPU's fp32 convolution and a bf16 output must
equal that result rounded once; a misplaced tap, row, swizzle or epilogue column cannot hide behind a tolerance.

Which kernel a case runs is not re-derived here: bfhip_conv2d_launch_choice / bfhip_conv2d_wgrad_choice answer with the launch
path's own functions, knobs and CU count (csrc/conv2d.hip, csrc/conv2d_wgrad.hip)."""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

#        N   H    W   Cin Cout k  s  p  d
CASES = [(1, 7, 9, 16, 24, 3, 1, 1, 1),          # one partial tile, M = 63
         (2, 19, 23, 40, 72, 3, 2, 1, 1),        # K pieces straddle taps (Cin = 40), parity classes
         (2, 19, 23, 72, 136, 1, 1, 0, 1),       # pointwise: 128-wide forward (8-wide last column tile), 128-wide dgrad, partial K step
         (2, 19, 23, 128, 40, 1, 1, 0, 1),       # pointwise: 64-wide forward, 128-wide dgrad
         (2, 19, 23, 40, 136, 1, 1, 0, 1),       # pointwise: 64-wide dgrad (GEMM columns = Cin = 40)
         (1, 20, 24, 64, 64, 3, 1, 2, 2),        # dilation 2
         (1, 21, 25, 16, 24, 3, 2, 2, 2),        # strided plain transposed gather: stride 2 with dilation 2
         (1, 33, 35, 16, 16, 3, 8, 1, 1),        # ... and stride 8
         (1, 17, 19, 16, 16, 5, 4, 2, 1),        # parity classes with 1 / 2 / 4 taps, odd extents
         (2, 33, 47, 64, 128, 1, 2, 0, 1),       # 1x1 stride 2: three of four parity classes have no tap (zero fill)
         (8, 8, 8, 16, 24, 3, 1, 1, 1),          # OH * OW == 64: eight row wraps per 64-pixel step of the wide weight gradient
         (1, 18, 22, 72, 136, 3, 2, 1, 1),       # M = 99 < one tile; for the knob runs: wide on both sides (128 x 128 mode 2, 256 x 256 forward)
         (1, 24, 40, 160, 136, 3, 1, 1, 1),      # 128 x 64 tiles, two stages, modes 0 and 1
         (2, 128, 128, 72, 72, 3, 1, 1, 1),      # 128 x 128, one stage, modes 0 and 1 (256 tiles)
         (1, 128, 128, 136, 136, 1, 1, 1, 1),    # 1x1 with padding: implicit GEMM, 128 x 128, 8-wide second column tile
         (1, 128, 128, 136, 136, 3, 1, 1, 1),    # 128 x 128, two stages, modes 0 and 1 (20 K steps)
         (2, 64, 66, 136, 16, 3, 2, 1, 1),       # 128 x 128 mode 2 (and 128 x 64 two-stage forward)
         (2, 222, 222, 16, 232, 3, 1, 1, 1),     # 256 x 256, mode 0 (386 row tiles, 24 empty columns)
         (2, 222, 222, 232, 16, 3, 1, 1, 1),     # 256 x 256, mode 1
         (2, 222, 222, 232, 16, 3, 2, 1, 1)]     # 256 x 256, mode 2


def case_id(g):
    return "x".join(str(v) for v in g)


def out_hw(g):
    N, H, W, Cin, Cout, k, s, p, d = g
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def rows(g):
    """GEMM rows of the forward (output pixels)."""
    OH, OW = out_hw(g)
    return g[0] * OH * OW


# the cases a child process with non-default knobs runs (its knobs hold for the whole process)
TINY = [g for g in CASES if rows(g) <= 1100]


def variations(g):
    """[(bias, pitched, stats)] * 2: a variation fixed by the case's position in the table and its complement -- every forward runs
    with both, so every tile shape sees bias, pitches (ldx = Cin + 8, ldy = Cout + 24, ldg = Cout + 16) and stat_partial on and off."""
    i = CASES.index(g)
    v = (bool(i & 1), bool(i & 2), bool(i & 4))
    return [v, tuple(not b for b in v)]


def launch_choice(lib, direction, g, out_f32):
    """(pointwise, shape | BN, stages, mode, BM, BN, tiles_m, tiles_n) of bfhip_conv2d_fwd (0) / bfhip_conv2d_dgrad (1)."""
    N, H, W, Cin, Cout, k, s, p, d = g
    out = (ctypes.c_int32 * 8)()
    rc = lib.bfhip_conv2d_launch_choice(direction, N, H, W, Cin, Cout, k, k, s, p, d, int(out_f32), ctypes.addressof(out))
    assert rc == 0, lib.bfhip_last_error()
    return tuple(out)


def wgrad_choice(lib, g):
    """(shape, tiles_co, tiles_k, splits) of bfhip_conv2d_wgrad."""
    N, H, W, Cin, Cout, k, s, p, d = g
    out = (ctypes.c_int32 * 4)()
    rc = lib.bfhip_conv2d_wgrad_choice(N, H, W, Cin, Cout, k, k, s, p, d, ctypes.addressof(out))
    assert rc == 0, lib.bfhip_last_error()
    return tuple(out)


def variant(choice, out_f32):
    """The instantiation a choice names: (pointwise, shape | BN, stages, out_f32, mode)."""
    return (choice[0], choice[1], choice[2], int(out_f32), choice[3])


def variants_of(lib, cases):
    """{variant: [(case id, 'fwd' | 'dgrad')]} over both directions and both output types."""
    seen = {}
    for g in cases:
        for direction in (0, 1):
            for f32 in (0, 1):
                seen.setdefault(variant(launch_choice(lib, direction, g, f32), f32), []).append(
                    (case_id(g), "dgrad" if direction else "fwd"))
    return seen


# Every instantiation csrc/conv2d.hip compiles, as (pointwise, shape | BN, stages, out_f32, mode).
PW_VARIANTS = [(1, bn, 1, f32, mode) for bn in (64, 128) for f32 in (0, 1) for mode in (0, 1)]                      # conv_pw_kernel: 8
IG128_VARIANTS = [(0, sh, st, f32, mode) for sh in (0, 1) for st in (1, 2) for f32 in (0, 1) for mode in (0, 1, 2)]  # 128-row tiles: 24
IG256_VARIANTS = [(0, 2, 2, 0, mode) for mode in (0, 1, 2)]                                                          # 256 x 256: 3
ALL_VARIANTS = PW_VARIANTS + IG128_VARIANTS + IG256_VARIANTS
# the parity-class data gradient always takes one stage by rule: its two-stage kernels need BFHIP_CONV_SINGLE_STAGE=0
KNOB_ONLY_VARIANTS = [(0, sh, 2, f32, 2) for sh in (0, 1) for f32 in (0, 1)]

# Child processes with non-default knobs (the knobs are function-local statics: fixed per process), the TINY cases only; `expect`:
# the variants the child must reach, read through the query inside the child.
CHILDREN = {
    # two-stage kernels everywhere (the parity classes included), 128 x 128 and 256 x 256 tiles where M is smaller than one tile,
    # the 256 x 256 tile's second statistics row beyond the last row block
    "A": (dict(BFHIP_CONV_SINGLE_STAGE="0", BFHIP_CONV_SMALL_GRID="0", BFHIP_CONV_QUANT="0", BFHIP_CONV_TILE256="2"),
          PW_VARIANTS + [(0, 0, 2, f32, mode) for f32 in (0, 1) for mode in (0, 1, 2)] +
          [(0, 1, 2, 0, 0), (0, 1, 2, 0, 2), (0, 1, 2, 1, 0), (0, 1, 2, 1, 1), (0, 1, 2, 1, 2), (0, 2, 2, 0, 0), (0, 2, 2, 0, 1)]),
    # one stage with long K loops, strided plain transposed gather for every strided case, 1x1 layers on the implicit GEMM
    "B": (dict(BFHIP_CONV_SINGLE_STAGE="2", BFHIP_CONV_DGRAD_PARITY="0", BFHIP_CONV_PW_MAXC="0"),
          [(0, 0, 1, f32, mode) for f32 in (0, 1) for mode in (0, 1)]),   # (the small-grid rule keeps every TINY case on 128 x 64)
}

# ------------------------------------------------------------------------------------------------ operands and reference
SENT = float(2 ** 20)   # pre-fill of every output buffer: exact in bf16 and fp32, far above any result of these operands
GUARD = 64              # pixels (rows of the output pitch) of guard band after the last pixel
POISON = 3.0            # what the unused columns of a pitched INPUT hold: a kernel that reads them gets a wrong sum, not a zero


@functools.lru_cache(maxsize=2)
def reference(g):
    """Integer operands of a case and its fp32 convolution on the CPU (forward without bias, data and weight gradient), all as
    channels-last matrices [pixels, channels]; computed once per case and shared (read-only) by every check of the case."""
    N, H, W, Cin, Cout, k, s, p, d = g
    rng = np.random.default_rng(1000 + sum((i + 1) * v for i, v in enumerate(g)))
    x = torch.from_numpy(rng.integers(-3, 4, (N, Cin, H, W)).astype(np.float32)).requires_grad_(True)
    w = torch.from_numpy(rng.integers(-2, 3, (Cout, Cin, k, k)).astype(np.float32)).requires_grad_(True)
    y = F.conv2d(x, w, None, stride=s, padding=p, dilation=d)
    dy = torch.from_numpy(rng.integers(-2, 3, tuple(y.shape)).astype(np.float32))
    y.backward(dy)
    bias = torch.from_numpy(rng.integers(-4, 5, (Cout,)).astype(np.float32))
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()  # noqa: E731
    ohwi = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()                           # noqa: E731
    r = types.SimpleNamespace(x=nhwc(x), w=ohwi(w), dy=nhwc(dy), bias=bias, y=nhwc(y), dx=nhwc(x.grad), dw=ohwi(w.grad))
    assert max(float(t.abs().max()) for t in (r.y, r.dx, r.dw)) + 4 < 2 ** 24      # exactness of every sum
    # statistics of the un-biased output per 128 GEMM rows; exact in fp32 as long as every sum of squares stays below 2^24
    M = r.y.shape[0]
    nblk = (M + 127) // 128
    yp = torch.zeros((nblk * 128, Cout), dtype=torch.float64)
    yp[:M] = r.y.double()
    yp = yp.view(nblk, 128, Cout)
    r.stat = torch.stack([yp.sum(1), (yp * yp).sum(1)], 1)                          # [nblk][2][Cout], fp64
    return r


def _dev_in(src, ld, off, dev):
    """bf16 device matrix [rows, ld] that holds `src` in columns [off, off + C) and POISON elsewhere; returns (buffer, pointer of
    the slice)."""
    buf = torch.full((src.shape[0], ld), POISON, dtype=torch.bfloat16, device=dev)
    buf[:, off:off + src.shape[1]] = src.to(dev)
    return buf, buf.data_ptr() + 2 * off


def _dev_out(rows, ld, dtype, dev):
    return torch.full((rows + GUARD, ld), SENT, dtype=dtype, device=dev)


def _check_out(buf, rows, C, want, what):
    got = buf[:rows, :C]
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i, j = (int(v) for v in bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at row %d column %d: got %r, want %r" %
                             (what, bad.shape[0], got.numel(), i, j, float(got[i, j]), float(want[i, j])))
    assert bool((buf[:rows, C:] == SENT).all()), what + ": columns beyond the channels were written"
    assert bool((buf[rows:] == SENT).all()), what + ": the guard band after the last pixel was written"


def _dtype(out_f32):
    return torch.float32 if out_f32 else torch.bfloat16


def check_forward(dev, g, out_f32, bias, pitch, stats):
    from bevfusion_amd import _lib
    N, H, W, Cin, Cout, k, s, p, d = g
    r = reference(g)
    M = r.y.shape[0]
    OH, OW = out_hw(g)
    what = "forward %s %s bias=%d pitch=%d stats=%d" % (case_id(g), "f32" if out_f32 else "bf16", bias, pitch, stats)
    ldx, ldy = (Cin + 8, Cout + 24) if pitch else (Cin, Cout)
    xb, xp = _dev_in(r.x, ldx, 8 if pitch else 0, dev)
    wd = r.w.to(dev).to(torch.bfloat16)
    bd = r.bias.to(dev) if bias else None
    y = _dev_out(M, ldy, _dtype(out_f32), dev)
    nblk = _lib.load().bfhip_conv2d_stat_rows(N, OH, OW)
    assert nblk == (M + 127) // 128
    st = torch.full((nblk + 1, 2, Cout), SENT, dtype=torch.float32, device=dev) if stats else None   # one guard row
    _lib.call("bfhip_conv2d_fwd", xp, ldx, wd.data_ptr(), _lib.ptr(bd), y.data_ptr(), ldy, N, H, W, Cin, Cout, k, k, s, p, d,
              int(out_f32), _lib.ptr(st), _lib.stream_of(xb))
    want = (r.y + r.bias) if bias else r.y          # integers: the bias joins the fp32 accumulator before the single rounding
    _check_out(y, M, Cout, want.to(dev).to(_dtype(out_f32)), what)
    if stats:
        assert float(r.stat[:, 1].max()) < 2 ** 24, "%s: sums of squares beyond 2^24, shrink the case's value range" % what
        assert torch.equal(st[:nblk], r.stat.float().to(dev)), what + ": stat_partial"
        assert bool((st[nblk] == SENT).all()), what + ": stat_partial row beyond bfhip_conv2d_stat_rows was written"


def check_dgrad(dev, g, out_f32, pitch):
    """bfhip_conv2d_dgrad; returns the whole output buffer (guard band included) for bit comparisons with bfhip_conv2d_dgrad_wt."""
    from bevfusion_amd import _lib
    N, H, W, Cin, Cout, k, s, p, d = g
    r = reference(g)
    what = "dgrad %s %s pitch=%d" % (case_id(g), "f32" if out_f32 else "bf16", pitch)
    ldg, ldx = (Cout + 16, Cin + 8) if pitch else (Cout, Cin)
    gb, gp = _dev_in(r.dy, ldg, 8 if pitch else 0, dev)
    wd = r.w.to(dev).to(torch.bfloat16)
    dx = _dev_out(N * H * W, ldx, _dtype(out_f32), dev)
    nws = _lib.load().bfhip_conv2d_dgrad_workspace_bytes(Cin, Cout, k, k)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _lib.call("bfhip_conv2d_dgrad", gp, ldg, wd.data_ptr(), dx.data_ptr(), ldx, N, H, W, Cin, Cout, k, k, s, p, d, int(out_f32),
              ws.data_ptr(), nws, _lib.stream_of(gb))
    # pixels of parity classes no tap reaches are zeros of the reference: the sentinel must not show through
    _check_out(dx, N * H * W, Cin, r.dx.to(dev).to(_dtype(out_f32)), what)
    return dx


def check_wgrad(dev, g, dw_bf16, pitch):
    from bevfusion_amd import _lib
    N, H, W, Cin, Cout, k, s, p, d = g
    r = reference(g)
    OH, OW = out_hw(g)
    what = "wgrad %s %s pitch=%d" % (case_id(g), "bf16" if dw_bf16 else "f32", pitch)
    ldx, ldg = (Cin + 8, Cout + 16) if pitch else (Cin, Cout)
    xb, xp = _dev_in(r.x, ldx, 8 if pitch else 0, dev)
    gb, gp = _dev_in(r.dy, ldg, 8 if pitch else 0, dev)
    nws = _lib.load().bfhip_conv2d_wgrad_workspace_bytes(N, OH, OW, Cin, Cout, k, k)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    dw = _dev_out(Cout, k * k * Cin, _dtype(not dw_bf16), dev)
    _lib.call("bfhip_conv2d_wgrad", xp, ldx, gp, ldg, dw.data_ptr(), N, H, W, Cin, Cout, k, k, s, p, d, int(dw_bf16),
              ws.data_ptr(), nws, _lib.stream_of(xb))
    _check_out(dw, Cout, k * k * Cin, r.dw.reshape(Cout, -1).to(dev).to(_dtype(not dw_bf16)), what)


PARTS = ("fwd", "dgrad", "wgrad")


def check_case(dev, g, part):
    """Everything the exact test asks of one case: both output types, the case's variation and its complement."""
    for i, (bias, pitch, stats) in enumerate(variations(g)):
        for f32 in (0, 1):
            if part == "fwd":
                check_forward(dev, g, f32, bias, pitch, stats)
            elif part == "dgrad":
                check_dgrad(dev, g, f32, pitch)
            elif f32 == i:      # weight gradient: fp32 dW with the variation's pitches, bf16 dW with the complement's
                check_wgrad(dev, g, f32, pitch)


def check_addend(dev, g, addend_stride, mode):
    """Data gradient of a pointwise case with the fused addend (bf16 output): bf16(float(bf16(acc)) + float(addend)); with
    addend_stride 2 the addend lives on the even pixels' grid and only they receive it.  mode: 'dense' (ldx = Cin), 'pitch'
    (ldx = Cin + 8), 'pair' (addend base 4 bytes past a 16-byte boundary: the epilogue's 4-byte tail path), 'odd' (ldx = Cin + 1:
    rows of dx alternate between 4- and 2-byte alignment, its 2-byte tail path)."""
    from bevfusion_amd import _lib
    N, H, W, Cin, Cout, k, s, p, d = g
    assert _lib.load().bfhip_conv2d_dgrad_fuses_addend(k, k, s, p, 0) == 1
    r = reference(g)
    what = "dgrad + addend %s addend_stride=%d %s" % (case_id(g), addend_stride, mode)
    AH, AW = ((H + 1) // 2, (W + 1) // 2) if addend_stride == 2 else (H, W)
    rng = np.random.default_rng(7 + addend_stride)
    add = torch.from_numpy(rng.integers(-100, 101, (N, AH, AW, Cin)).astype(np.float32))   # exact in bf16
    acc = r.dx.view(N, H, W, Cin).to(torch.bfloat16).float()
    if addend_stride == 2:
        acc[:, ::2, ::2] += add
    else:
        acc += add
    want = acc.to(torch.bfloat16).view(-1, Cin)
    ldx = {"dense": Cin, "pitch": Cin + 8, "pair": Cin, "odd": Cin + 1}[mode]
    off = 2 if mode == "pair" else 0
    ab = torch.zeros(add.numel() + 8, dtype=torch.bfloat16, device=dev)
    ab[off:off + add.numel()] = add.flatten().to(dev)
    gb, gp = _dev_in(r.dy, Cout, 0, dev)
    wt = r.w.permute(3, 1, 2, 0).contiguous().to(dev).to(torch.bfloat16)     # [Cin][KH][KW][Cout]
    dx = _dev_out(N * H * W, ldx, torch.bfloat16, dev)
    _lib.call("bfhip_conv2d_dgrad_wt", gp, Cout, wt.data_ptr(), ab.data_ptr() + 2 * off, addend_stride, dx.data_ptr(), ldx,
              N, H, W, Cin, Cout, k, k, s, p, d, 0, _lib.stream_of(gb))
    _check_out(dx, N * H * W, Cin, want.to(dev), what)


def child_main(name):
    """Body of a knob child: the query must name the variants the child exists for, then every TINY case runs the same checks as
    the parent."""
    import bevfusion_amd  # noqa: F401
    from bevfusion_amd import _lib
    env, expect = CHILDREN[name]
    assert all(os.environ.get(k) == v for k, v in env.items()), "child %s started without its knobs" % name
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    seen = variants_of(_lib.load(), TINY)
    assert set(seen) == set(expect), "child %s on %d CUs: missing %s, unexpected %s" % (
        name, cus, sorted(set(expect) - set(seen)), sorted(set(seen) - set(expect)))
    lib = _lib.load()
    both = [(launch_choice(lib, direction, g, f32), g, direction, f32) for g in TINY for direction in (0, 1) for f32 in (0, 1)]
    if name == "A":
        assert all(c[2] == 2 for c, g, _, _ in both if not c[0]), "a one-stage implicit GEMM under BFHIP_CONV_SINGLE_STAGE=0"
        # a 128 x 128 and a 256 x 256 launch of one row tile that M does not fill; the latter with one row of statistics, so the
        # tile's second partial row lies beyond bfhip_conv2d_stat_rows
        assert any(c[1] == 1 and not c[0] and direction == 0 and c[6] == 1 and rows(g) < 128 for c, g, direction, _ in both)
        assert any(c[1] == 2 and direction == 0 and c[6] == 1 and rows(g) <= 128 for c, g, direction, _ in both)
    else:
        assert all(not c[0] and c[2] == 1 for c, _, _, _ in both), "pointwise or two-stage launch under child B's knobs"
        assert all(c[3] == 1 for c, _, direction, _ in both if direction == 1), "parity classes under BFHIP_CONV_DGRAD_PARITY=0"
        assert {g[6] for _, g, direction, _ in both if direction == 1} >= {2, 4, 8}              # strided plain transposed gather
        assert any(g[5] == 1 and g[6] == 1 and g[7] == 0 for g in TINY)                           # 1x1 layers on the implicit GEMM
        assert any((g[5] * g[5] * g[3] // 8 + 7) // 8 > 18 for g in TINY)                         # a K loop beyond the 18-step rule
    for g in TINY:
        for part in PARTS:
            check_case(dev, g, part)
    torch.cuda.synchronize()
    print("child %s ok: %d cases, %d variants" % (name, len(TINY), len(seen)))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child_main(sys.argv[1])
