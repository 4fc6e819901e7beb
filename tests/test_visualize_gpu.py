"""GPU: csrc/visualize.hip against the specification of bevfusion_amd.visualize, torch.equal, on every case of
tests/visualize_cases.py and on kernel-only shapes: several tiles, tile borders, many segments, the real shape."""
import numpy as np
import pytest
import torch

import visualize_cases as cases
from bevfusion_amd import visualize as vz

pytestmark = pytest.mark.gpu


def to_dev(kw, dev):
    out = dict(kw)
    for k in ("frames", "points"):
        if k in out:
            out[k] = torch.from_numpy(np.ascontiguousarray(out[k])).to(dev)
    return out


def both(fn, kw, dev):
    """(kernel result on the device, the specification's on the host), with PATHS checked each way."""
    before = dict(vz.PATHS)
    got = fn(**to_dev(kw, dev))
    assert vz.PATHS["kernel"] == before["kernel"] + 1 and vz.PATHS["torch"] == before["torch"], "the kernel path did not run"
    want = fn(**kw)
    assert vz.PATHS["torch"] == before["torch"] + 1
    assert got.is_cuda and got.dtype == torch.uint8
    return got, want


@pytest.mark.parametrize("name", cases.CAMERA_CASES)
def test_camera_cases(dev, name):
    got, want = both(vz.render_cameras, cases.camera_case(name), dev)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("name", sorted(cases.COVERAGE))
def test_coverage_cases(dev, name):
    got, want = both(vz.render_bev, cases.coverage_case(name), dev)
    assert torch.equal(got.cpu(), want)
    assert np.array_equal((got.cpu().numpy() == np.array([255, 0, 0], np.uint8)).all(-1), cases.canvas(cases.COVERAGE[name][2]))


@pytest.mark.parametrize("name", cases.BEV_CASES)
def test_bev_cases(dev, name):
    got, want = both(vz.render_bev, cases.bev_case(name), dev)
    assert torch.equal(got.cpu(), want)


def test_overflow_trap(dev):
    got, want = both(vz.render_cameras, cases.trap_case(), dev)
    assert torch.equal(got.cpu(), want) and (want.numpy() != cases.trap_case()["frames"][0]).any()


@pytest.mark.parametrize("n_views,scale", [(2, 1), (6, 1), (6, 2), (2, 4)])
def test_frames_larger_than_a_tile(dev, n_views, scale):
    """70 x 130: three tile rows of 32 x 8 output pixels and a remainder both ways; long boxes cross the tile borders."""
    L, K = cases.rig(n_views, f=60.0, cx=65.0, cy=35.0, shape=(3, 4))
    b = cases.ring_boxes(14, seed=20 + n_views, dims=((2.0, 1.0, 1.0), (9.0, 3.0, 3.0)))
    kw = dict(frames=cases.frames(n_views, 70, 130, seed=n_views), boxes=b, colors=cases.colors(14), lidar2cam=L, cam2img=K,
              thickness=2.5, scale=scale)
    got, want = both(vz.render_cameras, kw, dev)
    assert torch.equal(got.cpu(), want)
    assert (vz.render_cameras(**dict(kw, boxes=b[:0], colors=kw["colors"][:0])) != want).any()


def test_more_segments_than_one_chunk(dev):
    """600 small boxes, 7200 records a view: 29 LDS chunks; 48 x 64 frames."""
    L, K = cases.rig(2, f=40.0, cx=32.0, cy=24.0)
    b = cases.ring_boxes(600, seed=31, r=(3.0, 20.0), dims=((0.3, 0.3, 0.3), (1.0, 1.0, 1.0)))
    kw = dict(frames=cases.frames(2, 48, 64, seed=8), boxes=b, colors=cases.colors(600), lidar2cam=L, cam2img=K, thickness=1.0)
    got, want = both(vz.render_cameras, kw, dev)
    assert torch.equal(got.cpu(), want)
    assert (want.numpy() != np.concatenate(list(kw["frames"]), 1)).mean() > 0.05


def test_inputs_the_kernel_does_not_take_run_the_specification(dev, monkeypatch):
    kw = cases.camera_case("five_views")
    want = vz.render_cameras(**kw)
    wide = torch.from_numpy(np.concatenate([kw["frames"], kw["frames"]], 2)).to(dev)
    before = dict(vz.PATHS)
    got = vz.render_cameras(**dict(kw, frames=wide[:, :, :37]))  # a non-contiguous device block
    assert vz.PATHS["torch"] == before["torch"] + 1 and vz.PATHS["kernel"] == before["kernel"]
    assert got.is_cuda and torch.equal(got.cpu(), want)
    got = vz.render_cameras(**dict(kw, frames=torch.from_numpy(kw["frames"])))  # a CPU tensor
    assert vz.PATHS["torch"] == before["torch"] + 2 and not got.is_cuda and torch.equal(got, want)
    monkeypatch.setattr(vz, "ENABLED", False)  # what BFHIP_VISUALIZE=0 sets
    got = vz.render_cameras(**to_dev(kw, dev))
    assert vz.PATHS["torch"] == before["torch"] + 3 and vz.PATHS["kernel"] == before["kernel"]
    assert got.is_cuda and torch.equal(got.cpu(), want)
    bev = cases.bev_case("cloud")
    got = vz.render_bev(**to_dev(bev, dev))
    assert vz.PATHS["torch"] == before["torch"] + 4 and torch.equal(got.cpu(), vz.render_bev(**bev))


def test_real_shape_against_the_specification_on_the_device(dev, monkeypatch):
    """6 x 900 x 1600, 200 boxes, scale 3, the nominal rig; the specification's pixels are computed on the device."""
    from bevfusion_amd import synthetic
    rig = synthetic.camera_rig(batch=1)
    boxes, _ = synthetic.gt_boxes(seed=3000, n=200)
    frames = torch.from_numpy(synthetic.camera_images_u8(batch=1, views=6, h=900, w=1600, seed=2001)[0].transpose(0, 2, 3, 1).copy()).to(dev)
    assert tuple(frames.shape) == (6, 900, 1600, 3) and len(boxes) == 200
    kw = dict(frames=frames, boxes=boxes, colors=cases.colors(200), lidar2cam=np.linalg.inv(rig["camera2lidar"][0].astype(np.float64)),
              cam2img=rig["camera_intrinsics"][0], scale=3)
    got = vz.render_cameras(**kw)
    assert vz.PATHS["kernel"] >= 1 and tuple(got.shape) == (600, 1599, 3)
    monkeypatch.setattr(vz, "ENABLED", False)
    want = vz.render_cameras(**kw)
    assert want.is_cuda and torch.equal(got, want)
    plain = vz.render_cameras(**dict(kw, boxes=boxes[:0], colors=kw["colors"][:0]))
    assert (plain != want).any(-1).float().mean() > 0.002
