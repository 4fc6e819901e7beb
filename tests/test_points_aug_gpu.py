"""GPU: csrc/points_aug.hip against its specification (points_aug.torch_points_aug, evaluated on the host) bit for bit, the
reference's recorded draws through the kernel path, and the preprocessor's branch."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import points_aug_cases as cases
from bevfusion_amd import _lib
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor

pytestmark = pytest.mark.gpu

RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
FAR = [500.0, 500.0, 500.0, 501.0, 501.0, 501.0]       # rejects every point
WIDE = [-1e4, -1e4, -1e4, 1e4, 1e4, 1e4]               # keeps every point


def _block():
    return int(_lib.load().bfhip_points_aug_block())


def _rot(angle):
    return pa.rotation_matrix(angle)[0].numpy()


def _sample_specs():
    """(n, order, flips, range) per sample: every size class of the kernel (empty, one row, around a wave, blocks + 1 row,
    many blocks), both step orders and none, the four flip combinations, all rejected, all kept with and without a range."""
    b = _block()
    return [(0, "RTS", (0, 0), RANGE), (1, "RST", (0, 1), WIDE), (63, "RTS", (1, 0), RANGE), (64, "RST", (1, 1), RANGE),
            (65, None, (0, 0), RANGE), (3 * b + 1, "RTS", (0, 1), RANGE), (5000, "RST", (1, 0), RANGE),
            (300, "RTS", (1, 1), FAR), (2 * b, "RTS", (0, 0), None), (b + 7, "RST", (1, 1), WIDE), (700, None, (1, 0), None)]


_batches = {}


def _batch(C, shuffle):
    """(points on the host, plans, the specification's outputs on the host) -- made once per case."""
    key = (C, shuffle)
    if key not in _batches:
        rs = np.random.RandomState(100 + C)
        points, plans = [], []
        for i, (n, order, flips, rng) in enumerate(_sample_specs()):
            p = ((rs.rand(n, C) - 0.5) * np.array([130, 130, 10, 1, 1, 1, 1, 1][:C])).astype(np.float32)
            plan = pa.PointsAugPlan()
            if order is not None:
                plan.set_rts(_rot(0.1 + 0.3 * i), rs.normal(scale=0.5, size=3), 0.9 + 0.02 * i, order)
            if any(flips):
                plan.set_flip(*flips)
            if rng is not None:
                plan.set_range(rng)
            if shuffle:
                plan.set_shuffle(0x9E3779B97F4A7C15 * (i + 1))
            points.append(torch.from_numpy(p))
            plans.append(plan)
        want = [pa.torch_points_aug(p, plan) for p, plan in zip(points, plans)]
        _batches[key] = (points, plans, want)
    return _batches[key]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("C", [3, 4, 5])
def test_kernel_equals_the_specification_bit_for_bit(dev, C, shuffle):
    points, plans, want = _batch(C, shuffle)
    specs = _sample_specs()
    got = pa.fused_points_aug([p.to(dev) for p in points], plans)
    assert [int(g.shape[0]) for g in got] == [int(w.shape[0]) for w in want]  # the counts
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same_bits(g, w), "sample %d (n=%d)" % (i, specs[i][0])  # values and order
    kept = [int(w.shape[0]) for w in want]
    assert kept[7] == 0 and kept[8] == specs[8][0] and kept[9] == specs[9][0] and kept[1] == 1
    assert 0 < kept[5] < specs[5][0] and 0 < kept[6] < 5000
    base = got[0].untyped_storage().data_ptr()
    assert all(g.untyped_storage().data_ptr() == base for g in got)
    if shuffle:  # not the input order
        plain = _batch(C, False)[2]
        assert not torch.equal(want[6], plain[6]) and torch.equal(want[6][want[6][:, 0].argsort()], plain[6][plain[6][:, 0].argsort()])


def test_kernel_equals_torch_points_aug_on_the_device(dev):
    points, plans, want = _batch(5, True)
    for i in (5, 6):
        assert _same_bits(pa.torch_points_aug(points[i].to(dev), plans[i]), want[i])


def test_empty_batches_and_more_samples_than_one_launch_holds(dev):
    plan = pa.PointsAugPlan().set_range(RANGE).set_shuffle(3)
    got = pa.fused_points_aug([torch.zeros((0, 4), device=dev) for _ in range(3)], [plan] * 3)
    assert [tuple(g.shape) for g in got] == [(0, 4)] * 3
    rs = np.random.RandomState(7)
    sizes = [0, 5, 0, 300, 17, 0, 64, 1, 0, 0, 257, 2, 3, 90, 0, 31, 0, 513, 4, 0, 0, 70, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 0]
    assert len(sizes) > 32
    points = [torch.from_numpy(((rs.rand(n, 4) - 0.5) * np.array([130, 130, 10, 1])).astype(np.float32)) for n in sizes]
    plans = []
    for i in range(len(sizes)):
        p = pa.PointsAugPlan().set_rts(_rot(0.05 * i), [0.1 * i, -0.2, 0.3], 1.0 + 0.01 * i, "RTS" if i % 2 else "RST")
        p.set_flip(i % 2, i % 3 == 0).set_range(RANGE)
        plans.append(p.set_shuffle(i) if i % 4 < 2 else p)
    got = pa.fused_points_aug([p.to(dev) for p in points], plans)
    for i, (g, p, plan) in enumerate(zip(got, points, plans)):
        assert _same_bits(g, pa.torch_points_aug(p, plan)), i


def test_the_three_entries_agree_on_a_batch_without_paste_or_sweeps(dev):
    """One batch of 17 samples (one more than a launch holds) through bfhip_points_aug, bfhip_points_aug_paste with empty paste
    descriptors, and bfhip_points_aug_sweeps with n_segments = 0 everywhere, without and with empty paste descriptors: the same
    kept counts and the same bytes from all four, those of torch_points_aug."""
    C, sizes = 5, [0, 1, 255, 256, 257, 513, 100, 0, 300, 64, 65, 511, 512, 2, 700, 31, 400]
    B = len(sizes)
    assert B == 17
    rs = np.random.RandomState(17)
    points = [torch.from_numpy(((rs.rand(n, C) - 0.5) * np.array([130, 130, 10, 1, 1])).astype(np.float32)) for n in sizes]
    plans = [pa.PointsAugPlan().set_rts(_rot(0.2 * i - 1.0), [0.3, -0.1 * i, 0.2], 0.95 + 0.01 * i, "RTS" if i % 2 else "RST")
             .set_flip(i % 2, i % 3 == 0).set_range(RANGE).set_shuffle(1000 + i) for i in range(B)]
    want = [pa.torch_points_aug(p, plan) for p, plan in zip(points, plans)]
    assert any(0 < len(w) < n for w, n in zip(want, sizes))  # the range drops some rows
    on_dev = [p.to(dev) for p in points]
    descs = pa.descriptors(on_dev, plans)
    total = sum(sizes)
    nbytes = _lib.call_size("bfhip_points_aug_workspace_bytes", total, B)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    routes = {"points_aug": lambda tail: _lib.call("bfhip_points_aug", descs, *tail),
              "paste, empty": lambda tail: _lib.call("bfhip_points_aug_paste", descs, (pa._Paste * B)(), *tail),
              "sweeps": lambda tail: _lib.call("bfhip_points_aug_sweeps", descs, None, (pa._Sweeps * B)(), *tail),
              "sweeps + paste, empty": lambda tail: _lib.call("bfhip_points_aug_sweeps", descs, (pa._Paste * B)(), (pa._Sweeps * B)(), *tail)}
    for name, route in routes.items():
        out = torch.full((total, C), float("nan"), device=dev)
        kept = torch.full((B,), -1, dtype=torch.int32, device=dev)
        route((B, C, out.data_ptr(), kept.data_ptr(), work.data_ptr(), nbytes, _lib.stream_of(out)))
        assert kept.tolist() == [len(w) for w in want], name
        row = 0
        for i, (n, w) in enumerate(zip(sizes, want)):
            assert _same_bits(out[row:row + len(w)], w), (name, i)
            row += n


def test_golden_draws_through_the_kernel_path(dev):
    draws = list(range(cases.n_draws()))
    deferred = [cases.run(d, defer=True)[0] for d in draws]
    got = pa.fused_points_aug([x["points"].to(dev) for x in deferred], [x["points_aug_plan"] for x in deferred])
    for d, g in zip(draws, got):
        cases.assert_points_match(d, g.cpu().numpy())  # the reference's mask, values within the derived bound


_CHILD = """
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import points_aug_cases as cases
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor
assert not pa.ENABLED
torch.manual_seed(21)
deferred = [cases.run(d, defer=True, shuffle=True)[0] for d in range(cases.n_draws())]
pre = Det3DDataPreprocessor().to("cuda:0")
out = pre(dict(inputs=dict(points=[x["points"] for x in deferred], points_aug_plan=[x["points_aug_plan"] for x in deferred])))
assert pa.PATHS == dict(kernel=0, torch=1), pa.PATHS
assert all(t.is_cuda for t in out["inputs"]["points"])
torch.save([t.cpu() for t in out["inputs"]["points"]], sys.argv[1])
"""


def test_preprocessor_path_and_its_switch(dev):
    draws = list(range(cases.n_draws()))
    eager = [cases.run(d)[0]["points"] for d in draws]
    deferred = [cases.run(d, defer=True)[0] for d in draws]
    pre = Det3DDataPreprocessor().to(dev)
    before = dict(pa.PATHS)
    out = pre(dict(inputs=dict(points=[x["points"] for x in deferred], points_aug_plan=[x["points_aug_plan"] for x in deferred])))
    got = out["inputs"]["points"]
    assert pa.PATHS["kernel"] == before["kernel"] + 1 and pa.PATHS["torch"] == before["torch"]
    assert all(g.is_cuda and _same_bits(g, e) for g, e in zip(got, eager))  # the eager host transforms, moved to the device
    # with the shuffle, against BFHIP_POINTS_AUG=0 in a fresh process: the torch path, the same bits
    torch.manual_seed(21)
    shuffled = [cases.run(d, defer=True, shuffle=True)[0] for d in draws]
    got = pre.process_points([x["points"].to(dev) for x in shuffled], [x["points_aug_plan"] for x in shuffled])
    assert pa.PATHS["kernel"] == before["kernel"] + 2
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = _CHILD % dict(root=root, tests=os.path.join(root, "tests"))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.pt")
        r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, BFHIP_POINTS_AUG="0"), capture_output=True,
                           text=True, timeout=300, cwd=root)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        child = torch.load(path, weights_only=True)
    assert len(child) == len(got) and all(_same_bits(g, c) for g, c in zip(got, child))
    assert not _same_bits(got[0], eager[0]) and got[0].shape == eager[0].shape  # shuffled


def test_extract_pts_feat_accepts_the_result(dev):
    from bevfusion_amd import synthetic
    from bevfusion_amd.bevfusion import nuscenes_config
    from bevfusion_amd.registry import MODELS
    torch.manual_seed(0)
    model = MODELS.build(nuscenes_config(camera=False, lidar=True)).to(dev).eval()
    pts = [torch.from_numpy(synthetic.lidar_sweep(6000, seed=1000 + i)) for i in range(2)]
    plans = [pa.PointsAugPlan().set_rts(_rot(0.3 * (i + 1)), [0.2, -0.1, 0.05], 1.05, "RTS").set_flip(i, 1 - i).set_range(RANGE)
             .set_shuffle(40 + i) for i in range(2)]
    pre = Det3DDataPreprocessor().to(dev)
    out = pre(dict(inputs=dict(points=pts, points_aug_plan=plans)))["inputs"]
    assert all(_same_bits(g, pa.torch_points_aug(p, plan)) for g, p, plan in zip(out["points"], pts, plans))
    with torch.no_grad():
        feat = model.extract_pts_feat(out)
    assert feat.shape == (2, 256, 180, 180) and bool(torch.isfinite(feat).all()) and float(feat.abs().max()) > 0
