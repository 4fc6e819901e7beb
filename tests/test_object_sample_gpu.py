"""GPU: the paste variant of csrc/points_aug.hip (bfhip_points_aug_paste) against its specification
(points_aug.torch_points_aug) bit for bit, the reference's recorded ObjectSample draws through the preprocessor, the fallback
and the argument checks."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import object_sample_cases as cases
from bevfusion_amd import _lib
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor

pytestmark = pytest.mark.gpu

RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
BLOCK = 256
N, M = 2 * BLOCK + 37, 300  # the paste / original boundary (row 300) and the tail (row 849) both fall inside a workgroup


def _cloud(rs, n, C):
    return ((rs.rand(n, C) - 0.5) * np.array([130, 130, 10, 1, 1, 1, 1, 1][:C])).astype(np.float32)


def _boxes(rs, cloud, K, dims):
    """K boxes centred on points of the cloud's middle (so that each holds some that pass the range filter), bottom centre 1 m
    below them."""
    cloud = cloud[(np.abs(cloud[:, :2]) < 40).all(1) & (cloud[:, 2] > -3) & (cloud[:, 2] < 1)]
    at = cloud[rs.randint(0, len(cloud), K), :3] if len(cloud) else (rs.rand(K, 3).astype(np.float32) - 0.5) * 100
    b = np.concatenate([at - np.array([0, 0, 1.0], np.float32), rs.uniform(0.5, 1.0, (K, 3)) * np.array(dims), rs.uniform(-3.14, 3.14, (K, 1))], 1)
    return b.astype(np.float32)


def _rot(angle):
    return pa.rotation_matrix(angle)[0].numpy()


def _chain(plan, i, shuffle):
    plan.set_rts(_rot(0.2 + 0.3 * i), [0.3, -0.2 * i, 0.1], 0.95 + 0.02 * i, "RTS" if i % 2 else "RST")
    plan.set_flip(i % 2, (i // 2) % 2).set_range(RANGE)
    return plan.set_shuffle(0x9E3779B97F4A7C15 * (i + 1)) if shuffle else plan


_batches = {}


def _batch(C, shuffle):
    """One batch with every kind of sample: pastes of 1, 40 and 64 boxes on N originals with M pasted rows, a sample without
    a paste, one with pasted rows and no originals, one whose every original lies inside a box, one with boxes that hold
    nothing -> (points, plans, the specification's outputs), all on the host, made once per case."""
    key = (C, shuffle)
    if key not in _batches:
        rs = np.random.RandomState(40 + C)
        points, plans = [], []
        for i, (n, m, K, dims) in enumerate([(N, M, 1, (40, 30, 8)), (N, M, 40, (12, 9, 5)), (N, M, 64, (10, 8, 5)), (N, 0, 0, None),
                                             (0, M, 3, (10, 8, 5)), (BLOCK + 9, 70, 2, None), (BLOCK, 1, 5, (0.01, 0.01, 0.01))]):
            p = _cloud(rs, n, C)
            plan = pa.PointsAugPlan()
            if K:
                boxes = _boxes(rs, p, K, dims) if dims else np.array([[0, 0, -50, 400, 400, 100, 0.3], [5, 5, -1, 2, 2, 2, 0]], np.float32)
                plan.set_paste(_cloud(rs, m, C), boxes)
            points.append(torch.from_numpy(p))
            plans.append(_chain(plan, i, shuffle))
        want = [pa.torch_points_aug(p, plan) for p, plan in zip(points, plans)]
        _batches[key] = (points, plans, want)
    return _batches[key]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def _check_cases(points, plans, want, shuffle):
    """The cases are what they claim to be: boxes dropped some but not all originals; only pasted rows are left where every
    original was inside a box; boxes that hold nothing dropped nothing (host only)."""
    unpasted = [pa.PointsAugPlan() for _ in plans]
    for u, plan in zip(unpasted, plans):
        for k in pa.PointsAugPlan.__slots__:
            setattr(u, k, getattr(plan, k) if k not in pa.PointsAugPlan._PASTE else None)
    alone = [int(pa.torch_points_aug(p, u).shape[0]) for p, u in zip(points, unpasted)]
    pasted_alone = [int(pa.torch_points_aug(torch.from_numpy(plan.paste_points), u).shape[0]) if plan.paste_points is not None else 0
                    for plan, u in zip(plans, unpasted)]
    kept = [int(w.shape[0]) for w in want]
    for i in (0, 1, 2):
        assert pasted_alone[i] < kept[i] < pasted_alone[i] + alone[i], i
    assert kept[3] == alone[3] and kept[4] == pasted_alone[4] > 0 and kept[5] == pasted_alone[5] > 0 and alone[5] > 0
    assert kept[6] == pasted_alone[6] + alone[6]
    if not shuffle:  # pasted rows first
        w = want[0]
        first = pa.torch_points_aug(torch.from_numpy(plans[0].paste_points), unpasted[0])
        assert _same_bits(w[:len(first)], first)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("C", [3, 4, 5])
def test_paste_kernel_equals_the_specification_bit_for_bit(dev, C, shuffle):
    points, plans, want = _batch(C, shuffle)
    assert int(_lib.load().bfhip_points_aug_block()) == BLOCK and pa.max_boxes() == 64
    assert pa.fused_supported([p.to(dev) for p in points], plans)
    got = pa.fused_points_aug([p.to(dev) for p in points], plans)
    assert [int(g.shape[0]) for g in got] == [int(w.shape[0]) for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same_bits(g, w), "sample %d" % i
    _check_cases(points, plans, want, shuffle)


def test_paste_kernel_equals_torch_points_aug_on_the_device(dev):
    points, plans, want = _batch(5, True)
    for i in (1, 5):
        assert _same_bits(pa.torch_points_aug(points[i].to(dev), plans[i]), want[i])


def test_more_samples_than_one_launch_holds(dev):
    rs = np.random.RandomState(3)
    sizes = [(300, 40, 3), (0, 0, 0), (5, 0, 0), (0, 17, 1), (257, 300, 7), (64, 1, 1), (1, 0, 2), (513, 255, 9), (90, 0, 0),
             (0, 0, 0), (31, 31, 31), (700, 2, 1), (256, 256, 4), (2, 600, 5), (0, 0, 0), (130, 65, 6), (511, 3, 2)]
    assert len(sizes) == 17
    points, plans = [], []
    for i, (n, m, K) in enumerate(sizes):
        p = _cloud(rs, n, 4)
        plan = pa.PointsAugPlan()
        if m or K:
            plan.set_paste(_cloud(rs, m, 4), _boxes(rs, p, K, (30, 20, 8)))
        points.append(torch.from_numpy(p))
        plans.append(_chain(plan, i, i % 3 == 0))
    got = pa.fused_points_aug([p.to(dev) for p in points], plans)
    for i, (g, p, plan) in enumerate(zip(got, points, plans)):
        assert _same_bits(g, pa.torch_points_aug(p, plan)), i


def test_too_many_boxes_or_another_width_take_the_torch_path(dev):
    rs = np.random.RandomState(9)
    p = _cloud(rs, 400, 5)
    for pasted, K in ((_cloud(rs, 50, 5), 65), (_cloud(rs, 50, 5), 64), (_cloud(rs, 50, 4), 3)):
        plan = pa.PointsAugPlan().set_paste(pasted, _boxes(rs, p, K, (12, 9, 5))).set_range(RANGE)
        before = dict(pa.PATHS)
        if pasted.shape[1] != 5:
            assert not pa.fused_supported([torch.from_numpy(p).to(dev)], [plan])
            continue
        got = pa.process_points([torch.from_numpy(p).to(dev)], [plan])
        path = "torch" if K > 64 else "kernel"
        assert pa.PATHS[path] == before[path] + 1 and sum(pa.PATHS.values()) == sum(before.values()) + 1
        assert got[0].is_cuda and _same_bits(got[0], pa.torch_points_aug(torch.from_numpy(p), plan))


@pytest.fixture(scope="module")
def cfg(tmp_path_factory):
    return cases.write_database(tmp_path_factory.mktemp("object_sample_db"))


_CHILD = """
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import torch
import object_sample_cases as cases
from bevfusion_amd import points_aug as pa
from bevfusion_amd.data_preprocessor import Det3DDataPreprocessor
assert not pa.ENABLED
cfg = cases.write_database(sys.argv[2])
deferred = cases.run(cfg, 1, defer=True)[0]
pre = Det3DDataPreprocessor().to("cuda:0")
out = pre(dict(inputs=dict(points=[x["points"] for x in deferred], points_aug_plan=[x["points_aug_plan"] for x in deferred])))
assert pa.PATHS == dict(kernel=0, torch=1), pa.PATHS
assert all(t.is_cuda for t in out["inputs"]["points"])
torch.save([t.cpu() for t in out["inputs"]["points"]], sys.argv[1])
"""


def test_golden_draws_through_the_preprocessor_and_its_switch(dev, cfg):
    pre = Det3DDataPreprocessor().to(dev)
    kept = None
    for d in range(cases.n_draws()):
        deferred, nxt = cases.run(cfg, d, defer=True)
        assert nxt == float(cases.golden()["draw%d_next_uniform" % d])
        before = dict(pa.PATHS)
        out = pre(dict(inputs=dict(points=[x["points"] for x in deferred], points_aug_plan=[x["points_aug_plan"] for x in deferred])))
        assert pa.PATHS["kernel"] == before["kernel"] + 1 and pa.PATHS["torch"] == before["torch"]
        for c, got in enumerate(out["inputs"]["points"]):
            assert got.is_cuda and _same_bits(got, torch.from_numpy(cases.reference(d, c)[2])), (d, c)  # the reference's bits
        if d == 1:
            kept = [g.cpu() for g in out["inputs"]["points"]]
    # BFHIP_POINTS_AUG=0 in a fresh process: the torch chain, the same bits
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    code = _CHILD % dict(root=root, tests=os.path.join(root, "tests"))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.pt")
        r = subprocess.run([sys.executable, "-c", code, path, tmp], env=dict(os.environ, BFHIP_POINTS_AUG="0"), capture_output=True,
                           text=True, timeout=300, cwd=root)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        child = torch.load(path, weights_only=True)
    assert len(child) == len(kept) and all(_same_bits(g, c) for g, c in zip(kept, child))


def test_invalid_arguments_are_rejected(dev):
    lib = _lib.load()
    pts = torch.zeros((8, 4), device=dev)
    table = torch.zeros(8 * 4 + 2 * 24, device=dev)
    out, kept = torch.empty((16, 4), device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = _lib.call_size("bfhip_points_aug_workspace_bytes", 16, 1)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    descs = pa.descriptors([pts], [pa.PointsAugPlan()])

    def call(points=table.data_ptr(), n_points=8, planes=table.data_ptr() + 4 * 32, n_boxes=2, pastes=True, C=4, out_ptr=out.data_ptr(),
             bytes_=nbytes, n_samples=1):
        p = (pa._Paste * 1)()
        p[0].points, p[0].n_points, p[0].planes, p[0].n_boxes = points, n_points, planes, n_boxes
        return lib.bfhip_points_aug_paste(descs, p if pastes else None, n_samples, C, out_ptr, kept.data_ptr(), work.data_ptr(), bytes_,
                                          _lib.stream_of(out))

    assert call() == 0  # the valid call the others depart from
    torch.cuda.synchronize()
    assert int(kept.item()) == 16  # 8 pasted rows + 8 originals: with all-zero planes every sign is 0, which is not < 0
    invalid = -1  # BFHIP_E_INVALID
    assert call(n_boxes=65) == invalid and call(n_boxes=-1) == invalid and call(n_points=-1) == invalid
    assert call(points=None) == invalid and call(planes=None) == invalid and call(pastes=False) == invalid
    assert call(points=table.data_ptr() + 2) == invalid and call(planes=table.data_ptr() + 1) == invalid
    assert call(C=2) == invalid and call(C=9) == invalid and call(n_samples=0) == invalid
    assert call(out_ptr=None) == invalid and call(bytes_=0) == invalid
    assert b"points_aug_paste" in lib.bfhip_last_error()
    assert call(points=None, n_points=0, planes=None, n_boxes=0) == 0  # an empty paste is a valid one
    torch.cuda.synchronize()
    assert int(kept.item()) == 8
