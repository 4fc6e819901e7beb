"""GPU: the sweep variants of csrc/points_aug.hip (bfhip_points_aug_sweeps) against their specification
(points_aug.torch_points_aug) bit for bit, the reference's recorded LoadPointsFromMultiSweeps runs through the preprocessor, the
fallback and the argument checks."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import multi_sweep_cases as cases
from bevfusion_amd import _lib
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor

pytestmark = pytest.mark.gpu

RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
BLOCK = 256
FULL = [n for n in cases.names() if n != "usedim"]


def _cloud(rs, n, C, close=0.1):
    """[n, C] over +-65 m; about `close` of the rows inside the 1 m square, and (n >= 2, close < 1) one row exactly on its
    border."""
    p = ((rs.rand(n, C) - 0.5) * np.array([130, 130, 10, 1, 1, 1, 1, 1][:C])).astype(np.float32)
    inside = rs.rand(n) < close
    p[inside, :2] = rs.uniform(-0.99, 0.99, (int(inside.sum()), 2)).astype(np.float32)
    if n >= 2 and close < 1:
        p[n // 2, :2] = [1.0, -0.5]
    return p


def _rigid(rs, S):
    m = np.tile(np.eye(4), (S, 1, 1))
    for i in range(S):
        a, b = rs.uniform(-np.pi, np.pi), rs.uniform(-0.05, 0.05)
        m[i, :3, :3] = (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @
                        np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]]))
        m[i, :3, 3] = rs.uniform(-8, 8, 3)
    return m


def _boxes(rs, K):
    b = np.concatenate([rs.uniform(-40, 40, (K, 2)), rs.uniform(-3, -1, (K, 1)), rs.uniform(6, 25, (K, 2)), rs.uniform(3, 8, (K, 1)),
                        rs.uniform(-3.14, 3.14, (K, 1))], 1)
    return b.astype(np.float32)


def _sample(rs, C, sizes, close=None, transform=True):
    """(points [sum sizes, C], a plan with the sweep step): sizes = rows of the keyframe and of every sweep; close: per sweep
    the fraction of rows inside the square (default 0.1)."""
    S = len(sizes) - 1
    close = close or [0.1] * S
    clouds = [_cloud(rs, sizes[0], C)] + [_cloud(rs, n, C, c) for n, c in zip(sizes[1:], close)]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    dt = (0.05 * (1 + np.arange(S)) + rs.uniform(-0.004, 0.004, S)).astype(np.float32)
    plan = pa.PointsAugPlan().set_sweeps(starts, _rigid(rs, S) if transform else None, dt, True)
    return np.concatenate(clouds, 0), plan


def _rot(angle):
    return pa.rotation_matrix(angle)[0].numpy()


def _chain(plan, i, shuffle):
    plan.set_rts(_rot(0.2 + 0.3 * i), [0.3, -0.2 * i, 0.1], 0.95 + 0.02 * i, "RTS" if i % 2 else "RST")
    plan.set_flip(i % 2, (i // 2) % 2).set_range(RANGE)
    return plan.set_shuffle(0x9E3779B97F4A7C15 * (i + 1)) if shuffle else plan


SIZES0 = [300, 37, 256, 0, 1, 219]  # boundaries 300, 337, 593, 593, 594 and the tail 813: all inside a 256-row workgroup
_batches = {}


def _batch(C, shuffle, paste):
    """One batch with every kind of sample (see _check_cases) -> (points, plans, the specification's outputs), all on the host,
    made once per case."""
    key = (C, shuffle, paste)
    if key not in _batches:
        rs = np.random.RandomState(70 + C)
        made = [_sample(rs, C, SIZES0),
                _sample(rs, C, [100, 50, 80], close=[1.0, 0.1]),                      # every row of sweep 1 is close
                _sample(rs, C, [40] + [20 + 3 * k for k in range(15)]),                # 16 segments
                (_cloud(rs, 300, C), pa.PointsAugPlan()),                              # no sweep step
                _sample(rs, C, [0, 130, 200]),                                         # an empty keyframe
                _sample(rs, C, [90, 90, 90], transform=False)]                         # padded copies: remove close, no transform
        made[5][0][90:] = np.tile(made[5][0][:90], (2, 1))
        points, plans = [], []
        for i, (p, plan) in enumerate(made):
            if paste and i in (0, 2):
                plan.set_paste(_cloud(rs, 300 if i == 0 else 33, C, 0.3), _boxes(rs, 5))
            points.append(torch.from_numpy(p))
            plans.append(_chain(plan, i, shuffle))
        want = [pa.torch_points_aug(p, plan) for p, plan in zip(points, plans)]
        _batches[key] = (points, plans, want)
    return _batches[key]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def _only(plan, keys):
    q = pa.PointsAugPlan()
    for k in keys:
        setattr(q, k, getattr(plan, k))
    return q


def _check_cases(points, plans, want, paste):
    """The cases are what they claim to be (host only)."""
    def close(p):
        return ((p[:, 0].abs() < 1) & (p[:, 1].abs() < 1)).numpy()

    p0, s0 = points[0], plans[0].sweep_starts
    assert list(s0) == [0, 300, 337, 593, 593, 594, 813] and len(p0) == 813
    m = 300 if paste else 0
    assert all((m + int(b)) % BLOCK for b in s0[1:]) and (m + 813) > 3 * BLOCK  # boundaries and tail inside a workgroup
    for a, b in zip(s0[1:-1], s0[2:]):  # remove-close drops some but not all rows of the sweeps that have more than one
        if b - a > 1:
            assert 0 < close(p0[a:b]).sum() < b - a
    assert close(p0[:300]).sum() > 0  # ... and the keyframe keeps its close rows
    alone = pa.torch_points_aug(p0, _only(plans[0], pa.PointsAugPlan._SWEEPS))
    assert len(alone) == 813 - sum(int(close(p0[a:b]).sum()) for a, b in zip(s0[1:-1], s0[2:]))
    assert (alone[:300, 4] == 0).all() and len(set(alone[300:, 4].tolist())) == 4  # dt per non-empty sweep
    assert not torch.equal(alone[300:, :3], p0[300:][~torch.from_numpy(close(p0[300:]))][:, :3])  # the sweeps moved
    assert 0 < len(want[0]) < len(alone) + m  # the range filter took some more
    p1, s1 = points[1], plans[1].sweep_starts
    assert close(p1[s1[1]:s1[2]]).all() and not close(p1[s1[2]:]).all()
    assert len(plans[2].sweep_starts) - 1 == 16 == pa.max_sweeps()
    assert plans[3].sweep_starts is None and plans[4].sweep_starts[1] == 0 and len(want[4]) > 0
    assert plans[5].sweep_l2s is None and plans[5].sweep_remove
    five = pa.torch_points_aug(points[5], _only(plans[5], pa.PointsAugPlan._SWEEPS))
    kept = int((~close(points[5][:90])).sum())
    assert len(five) == 90 + 2 * kept and torch.equal(five[90:90 + kept, :3], points[5][:90][~torch.from_numpy(close(points[5][:90]))][:, :3])
    if paste:
        assert len(plans[0].paste_points) == 300 and plans[2].paste_points is not None and plans[1].paste_points is None
        inside = pa.points_in_any_box(alone, torch.from_numpy(plans[0].paste_planes))
        assert inside[:300].any() and inside[300:].any() and not inside.all()  # the boxes hold keyframe rows and swept rows


@pytest.mark.parametrize("paste", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("C", [5, 6])
def test_sweep_kernels_equal_the_specification_bit_for_bit(dev, C, shuffle, paste):
    points, plans, want = _batch(C, shuffle, paste)
    assert int(_lib.load().bfhip_points_aug_block()) == BLOCK and pa.max_sweeps() == 16
    assert pa.fused_supported([p.to(dev) for p in points], plans)
    got = pa.fused_points_aug([p.to(dev) for p in points], plans)
    assert [int(g.shape[0]) for g in got] == [int(w.shape[0]) for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same_bits(g, w), "sample %d" % i
    _check_cases(points, plans, want, paste)


def test_sweep_kernels_equal_torch_points_aug_on_the_device(dev):
    points, plans, want = _batch(5, True, True)
    for i in (0, 5):
        assert _same_bits(pa.torch_points_aug(points[i].to(dev), plans[i]), want[i])


def test_more_samples_than_one_launch_holds(dev):
    rs = np.random.RandomState(5)
    sizes = [[300, 40, 3], [0], [5, 0, 0], [0, 17], [257, 300, 7], [64, 1, 1], None, [513, 255, 9, 1, 30], [90], None,
             [31, 31, 31], [700, 2, 1], [256, 256, 256], [2, 600, 5], [0, 0, 0], [130, 65, 6], [511, 3, 2]]
    assert len(sizes) == 17
    points, plans = [], []
    for i, sz in enumerate(sizes):
        p, plan = (_cloud(rs, 120, 5), pa.PointsAugPlan()) if sz is None else _sample(rs, 5, sz)
        if i % 4 == 1:
            plan.set_paste(_cloud(rs, 10 * i, 5, 0.3), _boxes(rs, 3))
        points.append(torch.from_numpy(p))
        plans.append(_chain(plan, i, i % 3 == 0))
    got = pa.fused_points_aug([p.to(dev) for p in points], plans)
    for i, (g, p, plan) in enumerate(zip(got, points, plans)):
        assert _same_bits(g, pa.torch_points_aug(p, plan)), i


def test_seventeen_segments_or_four_columns_take_the_torch_path(dev):
    rs = np.random.RandomState(11)
    for n_seg in (17, 16):
        p, plan = _sample(rs, 5, [50] + [10 + k for k in range(n_seg - 1)])
        plan.set_range(RANGE)
        before = dict(pa.PATHS)
        got = pa.process_points([torch.from_numpy(p).to(dev)], [plan])
        path = "torch" if n_seg > 16 else "kernel"
        assert pa.PATHS[path] == before[path] + 1 and sum(pa.PATHS.values()) == sum(before.values()) + 1
        assert got[0].is_cuda and _same_bits(got[0], pa.torch_points_aug(torch.from_numpy(p), plan))
    p, plan = _sample(rs, 5, [50, 20])
    assert not pa.fused_supported([torch.from_numpy(p[:, :4].copy()).to(dev)], [plan])        # no column 4
    assert not pa.fused_supported([torch.from_numpy(p[:60].copy()).to(dev)], [plan])          # rows that are not the plan's


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return cases.write_files(tmp_path_factory.mktemp("multi_sweep"))


_CHILD = """
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import multi_sweep_cases as cases
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor
assert not pa.ENABLED
files = cases.write_files(sys.argv[2])
deferred = [cases.run(files, name, defer=True, tensor=True)[0] for name in %(names)r]
pre = Det3DDataPreprocessor().to("cuda:0")
out = pre(dict(inputs=dict(points=[x["points"] for x in deferred], points_aug_plan=[x["points_aug_plan"] for x in deferred])))
assert pa.PATHS == dict(kernel=0, torch=1), pa.PATHS
assert all(t.is_cuda for t in out["inputs"]["points"])
torch.save([t.cpu() for t in out["inputs"]["points"]], sys.argv[1])
"""


def test_golden_runs_through_the_preprocessor_and_its_switch(dev, files):
    pre = Det3DDataPreprocessor().to(dev)
    deferred = []
    for name in FULL:
        data, nxt = cases.run(files, name, defer=True, tensor=True)
        assert nxt == float(cases.golden()[name + "_next_uniform"])
        deferred.append(data)
    before = dict(pa.PATHS)
    out = pre(dict(inputs=dict(points=[x["points"] for x in deferred], points_aug_plan=[x["points_aug_plan"] for x in deferred])))
    assert pa.PATHS["kernel"] == before["kernel"] + 1 and pa.PATHS["torch"] == before["torch"]
    kept = []
    for name, got in zip(FULL, out["inputs"]["points"]):
        assert got.is_cuda and _same_bits(got, torch.from_numpy(cases.reference(name))), name  # the reference's bits
        kept.append(got.cpu())
    # BFHIP_POINTS_AUG=0 in a fresh process: the torch chain, the same bits
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = _CHILD % dict(root=root, tests=os.path.join(root, "tests"), names=FULL)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.pt")
        r = subprocess.run([sys.executable, "-c", code, path, tmp], env=dict(os.environ, BFHIP_POINTS_AUG="0"), capture_output=True,
                           text=True, timeout=300, cwd=root)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        child = torch.load(path, weights_only=True)
    assert len(child) == len(kept) and all(_same_bits(g, c) for g, c in zip(kept, child))


def test_invalid_tables_are_rejected_and_nothing_is_launched(dev):
    lib = _lib.load()
    pts = torch.zeros((8, 5), device=dev)
    seg = np.zeros(2, pa.SEGMENT)
    seg["first"] = [0, 4]
    table = torch.from_numpy(seg.view(np.uint8).copy()).to(dev)
    spare = torch.zeros(8 + 112 * 17, dtype=torch.uint8, device=dev)
    out, kept = torch.empty((8, 5), device=dev), torch.full((1,), -7, dtype=torch.int32, device=dev)
    nbytes = _lib.call_size("bfhip_points_aug_workspace_bytes", 8, 1)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    descs = pa.descriptors([pts], [pa.PointsAugPlan()])

    def call(first=(0, 4, 8), n_segments=2, segments=table.data_ptr(), sweeps=True, C=5, out_ptr=out.data_ptr(), bytes_=nbytes,
             n_samples=1):
        w = (pa._Sweeps * 1)()
        w[0].segments, w[0].n_segments = segments, n_segments
        w[0].first[:len(first)] = list(first)
        return lib.bfhip_points_aug_sweeps(descs, None, w if sweeps else None, n_samples, C, out_ptr, kept.data_ptr(), work.data_ptr(),
                                           bytes_, _lib.stream_of(out))

    invalid = -1  # BFHIP_E_INVALID
    assert call(first=(0, 9, 8)) == invalid and b"boundary 2 (8) is below boundary 1 (9)" in lib.bfhip_last_error()
    assert call(first=(0, 4, 7)) == invalid and b"boundaries run from 0 to 7" in lib.bfhip_last_error()
    assert call(first=(1, 4, 8)) == invalid and b"boundaries run from 1 to 8" in lib.bfhip_last_error()
    assert call(n_segments=17, segments=spare.data_ptr()) == invalid and b"n_segments=17 (0 .. 16)" in lib.bfhip_last_error()
    assert call(n_segments=-1) == invalid and call(segments=None) == invalid
    assert call(C=4) == invalid and b"4 columns (5 .. 8" in lib.bfhip_last_error()
    assert call(C=9) == invalid
    assert call(segments=table.data_ptr() + 4) == invalid and b"segments not 8-byte aligned" in lib.bfhip_last_error()
    assert call(sweeps=False) == invalid and call(n_samples=0) == invalid and call(out_ptr=None) == invalid and call(bytes_=0) == invalid
    assert b"points_aug_sweeps" in lib.bfhip_last_error()
    torch.cuda.synchronize()
    assert int(kept.item()) == -7  # nothing was launched
    assert call() == 0  # the valid call the others depart from: two segments without flags keep every row
    torch.cuda.synchronize()
    assert int(kept.item()) == 8 and torch.equal(out, pts)
    assert call(n_segments=0, segments=None) == 0  # no sweep step: a valid sample
    torch.cuda.synchronize()
    assert int(kept.item()) == 8
