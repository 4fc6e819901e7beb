"""GPU: csrc/points_in_boxes.hip (bfhip_points_in_boxes_count / _gather) against its specification
(box_ops.torch_points_in_boxes) bit for bit, the reference's recorded database through the kernels, the builder on the device
against the builder on the host, the fallbacks and the argument checks."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import gt_database_cases as cases
import multi_sweep_cases as sweeps
from bevfusion_amd import _lib, box_ops, gt_database
from bevfusion_amd import points_aug as pa
from test_object_sample_gpu import _boxes, _cloud

pytestmark = pytest.mark.gpu

BLOCK = 256
NS = (0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 37)
KS = (0, 1, 63, 64, 65, 130)  # the chunk boundary of the LDS plane table and the word boundary of the mask


def _bits(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


_inputs = {}


def _case(n, K, C):
    """(points, boxes, the specification's counts / rows / centred rows / mask), made once on the host."""
    key = (n, K, C)
    if key not in _inputs:
        rs = np.random.RandomState(1000 * C + 10 * K + n % 7)
        p = _cloud(rs, n, C)
        b = _boxes(rs, p, K, (30, 22, 8)) if K else np.zeros((0, 7), np.float32)
        counts, rows, mask = box_ops.torch_points_in_boxes(p, b, return_mask=True)
        _, centred = box_ops.torch_points_in_boxes(p, b, center=True)
        _inputs[key] = (torch.from_numpy(p), b, counts, rows, centred, mask)
    return _inputs[key]


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("C", [3, 5, 8])
def test_kernel_equals_the_specification_bit_for_bit(dev, C, center):
    assert int(_lib.load().bfhip_points_in_boxes_block()) == BLOCK and box_ops.max_boxes() >= 256
    members = 0
    for n in NS:
        for K in KS:
            p, b, counts, rows, centred, mask = _case(n, K, C)
            before = dict(box_ops.PATHS)
            got_counts, got_rows, got_mask = box_ops.points_in_boxes(p.to(dev), b, center=center, return_mask=True)
            assert box_ops.PATHS["kernel"] == before["kernel"] + 1 and box_ops.PATHS["torch"] == before["torch"], (n, K)
            assert got_counts.dtype == torch.int32 and not got_counts.is_cuda and torch.equal(got_counts, counts), (n, K)
            assert got_rows.is_cuda and _bits(got_rows, centred if center else rows), (n, K)
            assert got_mask.shape == (n, K) and got_mask.dtype == torch.bool and torch.equal(got_mask.cpu(), mask), (n, K)
            again = box_ops.points_in_boxes(p.to(dev), b, center=center)  # without the mask: the words live in the workspace
            assert torch.equal(again[0], counts) and _bits(again[1], centred if center else rows), (n, K)
            assert torch.equal(box_ops.points_in_rbbox(p.to(dev), b).cpu(), mask), (n, K)
            members += int(counts.sum())
    assert members > 1000  # the boxes hold rows
    n, K = NS[-1], KS[-1]
    mask = _case(n, K, C)[5]
    assert int((mask.sum(1) > 1).sum()) > 0 and int((mask.sum(0) == 0).sum()) < K  # rows in several boxes; boxes with rows


def test_offsets_per_box_and_workgroup(dev):
    """The scan's output in the workspace: for every box the number of its rows in earlier workgroups."""
    n, K, C = NS[-1], 65, 5
    p, b, counts, _, _, mask = _case(n, K, C)
    planes, _ = box_ops.upload_table(pa.paste_planes(b), b[:, :3], dev)
    got_counts, words, (work, nbytes) = box_ops.kernel_count(p.to(dev), planes, want_words=True)
    blocks = (n + BLOCK - 1) // BLOCK
    per_block = torch.stack([mask[i * BLOCK:(i + 1) * BLOCK].sum(0) for i in range(blocks)], 1)  # [K, blocks]
    want = torch.cumsum(per_block, 1) - per_block
    got = work.cpu()[:K * blocks * 4].view(torch.int32).view(K, blocks)
    assert torch.equal(got.to(torch.int64), want) and torch.equal(got_counts.cpu(), counts)
    assert words.shape == (n, 2) and torch.equal(box_ops.unpack_words(words, K).cpu(), mask)
    assert nbytes == _lib.call_size("bfhip_points_in_boxes_workspace_bytes", n, K) and nbytes % 256 == 0


def test_special_boxes_and_a_nan_row(dev):
    rs = np.random.RandomState(5)
    p = _cloud(rs, 2 * BLOCK + 37, 5)
    p[300, 0] = np.nan
    p[17, 2] = np.nan
    some = _boxes(rs, p, 3, (30, 22, 8))
    boxes = np.concatenate([np.array([[0, 0, -50, 400, 400, 100, 0.3]], np.float32),          # holds every row
                            some[:1], some[:1],                                             # two identical boxes
                            np.array([[5, 5, -1, 0.01, 0.01, 0.01, 0], [300, 300, 0, 2, 2, 2, 1], [0, 0, -1, 0, 4, 4, 0.5]], np.float32),
                            some[1:]], 0)                                                   # three that hold nothing
    counts, rows = box_ops.torch_points_in_boxes(p, boxes, center=True)
    assert counts[0] == len(p) and counts[1] == counts[2] > 2 and counts[3:6].tolist() == [2, 2, 2]  # the two NaN rows are in every box
    got_counts, got_rows, got_mask = box_ops.points_in_boxes(torch.from_numpy(p).to(dev), boxes, center=True, return_mask=True)
    assert torch.equal(got_counts, counts) and _bits(got_rows, rows)
    assert bool(got_mask[300].all()) and bool(got_mask[17].all())
    starts = np.concatenate([[0], np.cumsum(counts.numpy())])
    assert _bits(got_rows[starts[1]:starts[2]], got_rows[starts[2]:starts[3]])


@pytest.mark.parametrize("f", range(4))
def test_golden_frames_through_the_kernel(dev, f):
    points, boxes, mask = cases.frame(f)
    want_counts, want_rows = cases.frame_rows(f)
    before = dict(box_ops.PATHS)
    counts, rows, got_mask = box_ops.points_in_boxes(torch.from_numpy(points).to(dev), boxes, center=True, return_mask=True)
    assert box_ops.PATHS["kernel"] == before["kernel"] + 1
    assert np.array_equal(counts.numpy(), want_counts) and np.array_equal(got_mask.cpu().numpy(), mask)
    assert _bits(rows, torch.from_numpy(want_rows))  # the reference's recorded bytes


def test_two_calls_give_identical_bytes(dev):
    p, b = _case(NS[-1], 130, 5)[:2]
    d = p.to(dev)
    a = box_ops.points_in_boxes(d, b, center=True, return_mask=True)
    c = box_ops.points_in_boxes(d, b, center=True, return_mask=True)
    assert torch.equal(a[0], c[0]) and _bits(a[1], c[1]) and torch.equal(a[2], c[2])


def _sweep_samples(root):
    """Three data_info dicts on the multi-sweep fixture's files: twelve sweeps (ten are drawn), three sweeps, none (padded)."""
    key_path, infos = sweeps.write_files(root)
    g = sweeps.golden()
    rs = np.random.RandomState(11)
    key = g["keyframe"]
    out = []
    for i, available in enumerate((12, 3, None)):
        K = (9, 70, 5)[i]
        boxes = np.concatenate([key[rs.randint(0, len(key), K), :3] - np.array([0, 0, 1.0], np.float32),
                                rs.uniform([2, 1.5, 1.5], [12, 6, 4], (K, 3)), rs.uniform(-3.14, 3.14, (K, 1)), rs.rand(K, 2)], 1)
        data = dict(sample_idx=40 + i, lidar_points=dict(lidar_path=key_path), timestamp=float(g["timestamp"]),
                    ann_info=dict(gt_bboxes_3d=boxes.astype(np.float32), gt_labels_3d=rs.randint(0, 3, K).astype(np.int64)))
        if available is not None:
            data["lidar_sweeps"] = infos[:available]
        out.append(data)
    return out


def _read_db(root, prefix):
    db = os.path.join(str(root), prefix + "_gt_database")
    with open(os.path.join(str(root), prefix + "_dbinfos_train.pkl"), "rb") as fh:
        raw = fh.read()
    return {name: open(os.path.join(db, name), "rb").read() for name in sorted(os.listdir(db))}, raw


@pytest.mark.parametrize("defer", [False, True])
def test_builder_on_the_device_writes_what_the_host_writes(dev, tmp_path, defer):
    samples = _sweep_samples(tmp_path)
    classes = ["car", "truck", "bus"]
    np.random.seed(4)
    host = gt_database.create_groundtruth_database(samples, gt_database.nuscenes_pipeline(defer=False), classes, str(tmp_path / "host"),
                                                   "nus", used_classes=["car", "bus"], device="cpu")
    before = dict(box_ops.PATHS)
    np.random.seed(4)
    got = gt_database.create_groundtruth_database(samples, gt_database.nuscenes_pipeline(defer=defer), classes, str(tmp_path / "dev"),
                                                  "nus", used_classes=["car", "bus"], device=dev)
    assert box_ops.PATHS["kernel"] == before["kernel"] + len(samples) and box_ops.PATHS["torch"] == before["torch"]
    host_files, host_pickle = _read_db(tmp_path / "host", "nus")
    dev_files, dev_pickle = _read_db(tmp_path / "dev", "nus")
    assert list(host_files) == list(dev_files) and len(host_files) == 84
    assert all(host_files[name] == dev_files[name] for name in host_files)
    assert host_pickle == dev_pickle and sorted(pickle.loads(dev_pickle)) == ["bus", "car"]
    assert sum(len(v) for v in host_files.values()) > 84 * 20 * 5  # the boxes hold points
    assert sorted(got) == sorted(host)


_CHILD = """
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import torch
from bevfusion_amd import box_ops
assert not box_ops.ENABLED
z = np.load(sys.argv[1])
counts, rows, mask = box_ops.points_in_boxes(torch.from_numpy(z["p"]).to("cuda:0"), z["b"], center=True, return_mask=True)
assert box_ops.PATHS == dict(kernel=0, torch=1), box_ops.PATHS
assert rows.is_cuda and mask.is_cuda
torch.save([counts.cpu(), rows.cpu(), mask.cpu()], sys.argv[2])
"""


def test_fallbacks_give_the_same_bits(dev, tmp_path):
    rs = np.random.RandomState(21)
    p = _cloud(rs, 2 * BLOCK + 37, 5)
    # more boxes than the kernels take
    K = box_ops.max_boxes() + 1
    b = _boxes(rs, p, K, (30, 22, 8))
    want = box_ops.torch_points_in_boxes(p, b, center=True, return_mask=True)
    before = dict(box_ops.PATHS)
    got = box_ops.points_in_boxes(torch.from_numpy(p).to(dev), b, center=True, return_mask=True)
    assert box_ops.PATHS["torch"] == before["torch"] + 1 and box_ops.PATHS["kernel"] == before["kernel"]
    assert got[1].is_cuda and torch.equal(got[0], want[0]) and _bits(got[1], want[1]) and torch.equal(got[2].cpu(), want[2])
    at_cap = box_ops.points_in_boxes(torch.from_numpy(p).to(dev), b[:K - 1], center=True)
    assert box_ops.PATHS["kernel"] == before["kernel"] + 1
    assert torch.equal(at_cap[0], want[0][:K - 1]) and _bits(at_cap[1], want[1][:int(want[0][:K - 1].sum())])
    # non-contiguous points
    wide = torch.from_numpy(_cloud(rs, 700, 8)).to(dev)
    view = wide[:, :5]
    assert not view.is_contiguous()
    before = dict(box_ops.PATHS)
    got = box_ops.points_in_boxes(view, b[:40], center=True)
    assert box_ops.PATHS["torch"] == before["torch"] + 1
    want = box_ops.points_in_boxes(view.contiguous(), b[:40], center=True)
    assert box_ops.PATHS["kernel"] == before["kernel"] + 1 and torch.equal(got[0], want[0]) and _bits(got[1], want[1])
    # BFHIP_POINTS_IN_BOXES=0 in a fresh process
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    np.savez(str(tmp_path / "in.npz"), p=p, b=b[:70])
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=root, tests=os.path.join(root, "tests")), str(tmp_path / "in.npz"),
                        str(tmp_path / "out.pt")], env=dict(os.environ, BFHIP_POINTS_IN_BOXES="0"), capture_output=True, text=True,
                       timeout=300, cwd=root)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    child = torch.load(str(tmp_path / "out.pt"), weights_only=True)
    mine = box_ops.points_in_boxes(torch.from_numpy(p).to(dev), b[:70], center=True, return_mask=True)
    assert torch.equal(child[0], mine[0]) and _bits(child[1], mine[1]) and torch.equal(child[2], mine[2].cpu())


def test_invalid_arguments_are_rejected(dev):
    lib = _lib.load()
    n, K, C = 300, 5, 4
    pts = torch.zeros((n, C), device=dev)
    planes = torch.zeros((K, 6, 4), device=dev)
    centers = torch.zeros((K, 3), device=dev)
    counts = torch.full((K,), -1, dtype=torch.int32, device=dev)
    nbytes = _lib.call_size("bfhip_points_in_boxes_workspace_bytes", n, K)
    work = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((8, C), device=dev)
    stream = _lib.stream_of(pts)
    cap = lib.bfhip_points_in_boxes_max_boxes()
    assert _lib.call_size("bfhip_points_in_boxes_workspace_bytes", n, cap + 1) == 0

    def count(points=pts.data_ptr(), n_=n, C_=C, planes_=planes.data_ptr(), K_=K, counts_=counts.data_ptr(), member=None,
              work_=work.data_ptr(), bytes_=nbytes):
        return lib.bfhip_points_in_boxes_count(points, n_, C_, planes_, K_, counts_, member, work_, bytes_, stream)

    def gather(points=pts.data_ptr(), n_=n, C_=C, centers_=centers.data_ptr(), K_=K, counts_=counts.data_ptr(), member=None, total=0,
               out_=out.data_ptr(), capacity=8, work_=work.data_ptr(), bytes_=nbytes):
        return lib.bfhip_points_in_boxes_gather(points, n_, C_, centers_, K_, counts_, member, total, out_, capacity, work_, bytes_, stream)

    invalid = -1  # BFHIP_E_INVALID
    assert count(C_=2) == invalid and count(C_=9) == invalid and count(K_=cap + 1) == invalid and count(K_=-1) == invalid
    assert count(points=None) == invalid and count(planes_=None) == invalid and count(counts_=None) == invalid
    assert count(n_=1 << 31) == invalid and count(n_=-1) == invalid
    assert count(points=pts.data_ptr() + 2) == invalid and count(member=work.data_ptr() + 4) == invalid
    assert count(work_=work.data_ptr() + 8) == invalid and count(bytes_=nbytes - 1) == invalid and count(work_=None) == invalid
    assert b"points_in_boxes_count" in lib.bfhip_last_error()
    torch.cuda.synchronize()
    assert counts.tolist() == [-1] * K  # nothing was launched
    assert count() == 0  # the valid call the others depart from: all-zero planes, every sign is 0, no row is inside
    torch.cuda.synchronize()
    assert counts.tolist() == [0] * K
    assert gather(C_=2) == invalid and gather(K_=cap + 1) == invalid and gather(points=None) == invalid and gather(counts_=None) == invalid
    assert gather(total=9) == invalid and gather(total=3, out_=None) == invalid and gather(total=1 << 31, capacity=1 << 32) == invalid
    assert gather(total=-1) == invalid and gather(bytes_=nbytes - 1) == invalid and gather(work_=None) == invalid
    assert gather(centers_=centers.data_ptr() + 1) == invalid and gather(n_=1 << 31) == invalid
    assert b"points_in_boxes_gather" in lib.bfhip_last_error()
    assert gather() == 0 and gather(centers_=None) == 0
    assert count(n_=0, points=None) == 0 and count(K_=0, planes_=None, counts_=None) == 0  # empty inputs are valid ones
    torch.cuda.synchronize()
