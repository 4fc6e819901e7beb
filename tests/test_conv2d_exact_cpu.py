"""CPU: the case table of the bit-exact convolution tests (conv_exact_cases.py) reaches every kernel csrc/conv2d.hip compiles.

bfhip_conv2d_launch_choice / bfhip_conv2d_wgrad_choice are host-only and answer with the launch path's own functions; without a
device the CU count is 256, the MI355X's.  If a chooser rule, a knob default or the table changes so that an instantiation is no
longer run by test_conv2d_exact_gpu.py, these tests fail here, before any GPU is involved."""
import json
import os
import subprocess
import sys

import bevfusion_amd  # noqa: F401
from bevfusion_amd import _lib

import conv_exact_cases as C

# (pointwise, tile shape (0 = 128x64, 1 = 128x128, 2 = 256x256; pointwise: tile width), stages, fp32 output, gather mode)
DEFAULT_REACHABLE = [
    # conv_pw_kernel<NI, F32, DIR>
    (1, 64, 1, 0, 0), (1, 64, 1, 0, 1), (1, 64, 1, 1, 0), (1, 64, 1, 1, 1),
    (1, 128, 1, 0, 0), (1, 128, 1, 0, 1), (1, 128, 1, 1, 0), (1, 128, 1, 1, 1),
    # conv_igemm_kernel, 128 x 64, one stage
    (0, 0, 1, 0, 0), (0, 0, 1, 0, 1), (0, 0, 1, 0, 2), (0, 0, 1, 1, 0), (0, 0, 1, 1, 1), (0, 0, 1, 1, 2),
    # 128 x 64, two stages (the parity classes always take one stage)
    (0, 0, 2, 0, 0), (0, 0, 2, 0, 1), (0, 0, 2, 1, 0), (0, 0, 2, 1, 1),
    # 128 x 128, one stage
    (0, 1, 1, 0, 0), (0, 1, 1, 0, 1), (0, 1, 1, 0, 2), (0, 1, 1, 1, 0), (0, 1, 1, 1, 1), (0, 1, 1, 1, 2),
    # 128 x 128, two stages
    (0, 1, 2, 0, 0), (0, 1, 2, 0, 1), (0, 1, 2, 1, 0), (0, 1, 2, 1, 1),
    # 256 x 256 (bf16 output only)
    (0, 2, 2, 0, 0), (0, 2, 2, 0, 1), (0, 2, 2, 0, 2),
]


def _no_conv_knobs():
    return not [k for k in os.environ if k.startswith("BFHIP_CONV_") or k.startswith("BFHIP_WGRAD_")]


def test_default_knobs_reach_every_default_reachable_kernel():
    assert _no_conv_knobs(), "this test describes the default knobs"
    assert len(DEFAULT_REACHABLE) == 31 == len(set(DEFAULT_REACHABLE))
    assert sorted(DEFAULT_REACHABLE + C.KNOB_ONLY_VARIANTS) == sorted(C.ALL_VARIANTS) and len(C.ALL_VARIANTS) == 35
    seen = C.variants_of(_lib.load(), C.CASES)
    assert sorted(seen) == sorted(DEFAULT_REACHABLE), (sorted(set(DEFAULT_REACHABLE) - set(seen)), sorted(set(seen) - set(DEFAULT_REACHABLE)))


def test_query_reports_the_tiles_of_the_launch():
    """Tile counts follow from the reported tile shape; the parity-class launch counts its row tiles class by class."""
    lib = _lib.load()
    for g in C.CASES:
        N, H, W, Cin, Cout, k, s, p, d = g
        for direction, M, cols in ((0, C.rows(g), Cout), (1, N * H * W, Cin)):
            pw, shape, stages, mode, BM, BN, tm, tn = C.launch_choice(lib, direction, g, 0)
            assert (BM, BN) == ((128, shape) if pw else {0: (128, 64), 1: (128, 128), 2: (256, 256)}[shape])
            assert tn == -(-cols // BN) and (mode == 0) == (direction == 0) and stages in (1, 2)
            if mode == 2:
                classes = [(len(range(a, H, s)), len(range(b, W, s))) for a in range(s) for b in range(s)]
                assert tm == sum(-(-N * hc * wc // BM) for hc, wc in classes if hc and wc)
            else:
                assert tm == -(-M // BM)
    strided = [g for g in C.CASES if g[6] > 1]
    assert {C.launch_choice(lib, 1, g, 0)[3] for g in strided if g[6] <= 4 and g[8] == 1} == {2}
    assert {C.launch_choice(lib, 1, g, 0)[3] for g in strided if g[6] > 4 or g[8] > 1} == {1}   # strided plain transposed gather
    assert len([g for g in strided if g[6] > 4 or g[8] > 1]) >= 2


def test_children_reach_the_knob_only_kernels_and_all_35_are_named():
    """The knobs are read once per process, so each knob set is queried in a child (host only).  Child A must name the four two-stage
    parity-class kernels no default rule reaches; parent and children together name every instantiation."""
    assert _no_conv_knobs()
    named = set(C.variants_of(_lib.load(), C.CASES))
    code = ("import sys, json; sys.path[:0] = %r; import bevfusion_amd; from bevfusion_amd import _lib; import conv_exact_cases as C; "
            "print(json.dumps(sorted(C.variants_of(_lib.load(), C.TINY))))" % [os.path.dirname(os.path.dirname(os.path.abspath(C.__file__))), os.path.dirname(os.path.abspath(C.__file__))])
    for name, (env, expect) in sorted(C.CHILDREN.items()):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        seen = {tuple(v) for v in json.loads(r.stdout.strip().splitlines()[-1])}
        assert seen == set(expect), (name, sorted(set(expect) - seen), sorted(seen - set(expect)))
        named |= seen
    assert set(C.KNOB_ONLY_VARIANTS) <= set(C.CHILDREN["A"][1])
    assert named == set(C.ALL_VARIANTS), sorted(set(C.ALL_VARIANTS) - named)
    assert all(C.rows(g) <= 1100 for g in C.TINY) and len(C.TINY) >= 10


def test_variations_cover_every_forward_tile_shape():
    """Bias, pitches and stat_partial each occur on and off on every forward tile shape: every case runs a variation and its
    complement."""
    for g in C.CASES:
        a, b = C.variations(g)
        assert all(x != y for x, y in zip(a, b))
    assert len({C.variations(g)[0] for g in C.CASES}) == 8


def test_weight_gradient_plans_of_the_table():
    lib = _lib.load()
    plans = {g: C.wgrad_choice(lib, g) for g in C.CASES}
    assert {p[0] for p in plans.values()} == {0, 1, 2}
    assert any(p[3] == 1 for p in plans.values()) and any(p[3] > 1 for p in plans.values())
    # a wide-kernel case with exactly 64 pixels per image: eight row wraps per 64-pixel step
    assert any(p[0] != 0 and C.out_hw(g)[0] * C.out_hw(g)[1] == 64 for g, p in plans.items())
    # several K panels with a partial last one
    assert any(p[2] > 1 and (g[5] * g[5] * g[3]) % (256 if p[0] == 1 else 128) != 0 for g, p in plans.items())
    for g, (shape, tiles_co, tiles_k, splits) in plans.items():
        N, H, W, Cin, Cout, k, s, p, d = g
        OH, OW = C.out_hw(g)
        assert tiles_co == -(-Cout // (256 if shape == 2 else 128)) and tiles_k == -(-k * k * Cin // (256 if shape == 1 else 128))
        assert 1 <= splits <= -(-C.rows(g) // 64)
        want = -(-(splits * Cout * k * k * Cin * 4) // 256) * 256
        assert lib.bfhip_conv2d_wgrad_workspace_bytes(N, OH, OW, Cin, Cout, k, k) == want, g


def test_queries_reject_what_the_launch_rejects():
    import ctypes
    lib = _lib.load()
    out = (ctypes.c_int32 * 8)()
    ok = lambda *a: lib.bfhip_conv2d_launch_choice(*a, ctypes.addressof(out))  # noqa: E731
    assert ok(0, 1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 0) == 0
    assert ok(2, 1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 0) != 0      # direction
    assert ok(0, 1, 8, 8, 12, 16, 3, 3, 1, 1, 1, 0) != 0      # channels not a multiple of 8
    assert ok(0, 1, 8, 8, 16, 16, 3, 3, 3, 1, 1, 0) != 0      # stride not a power of two
    assert ok(0, 1, 2, 2, 16, 16, 5, 5, 1, 0, 1, 0) != 0      # empty output
    assert lib.bfhip_conv2d_launch_choice(0, 1, 8, 8, 16, 16, 3, 3, 1, 1, 1, 0, None) != 0
    assert lib.bfhip_conv2d_wgrad_choice(1, 8, 8, 16, 16, 3, 3, 1, 1, 1, None) != 0
    assert lib.bfhip_conv2d_wgrad_choice(1, 2, 2, 16, 16, 5, 5, 1, 0, 1, ctypes.addressof(out)) != 0
