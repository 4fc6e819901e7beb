"""GPU: the device path of the JPEG encoder (csrc/jpeg_encode.hip) against its restatement (jpeg_encode.torch_jpeg_forward), the
host entropy encoder (csrc/jpeg_encode_host.h) and Pillow's recorded files, byte for byte.  No PIL needed: the recordings come
from tests/golden/jpeg_encode_cases.npz."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_encode_cases as ec

pytestmark = pytest.mark.gpu

RECORDED = ec.recorded()
GUARD = 64


@pytest.fixture(scope="module")
def je():
    from bevfusion_amd import jpeg_encode
    return jpeg_encode


@pytest.fixture(scope="module")
def jpeg():
    from bevfusion_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def pictures(dev):
    return [torch.from_numpy(ec.pixels(seed, w, h, noise)).to(dev) for _, seed, _, w, h, _, noise, _, _, _ in RECORDED]


@pytest.fixture(scope="module")
def host_files(je):
    """The host path's file of every recorded case, computed once."""
    return [je.encode(ec.pixels(seed, w, h, noise), q, sampling, 1) for _, seed, sampling, w, h, q, noise, _, _, _ in RECORDED]


@pytest.fixture(scope="module")
def fixture_frame(jpeg):
    return jpeg.decode(open(jc.FIXTURE, "rb").read())


def _specs(je):
    return [(w, h) + je.SAMPLINGS[sampling] + (je.quant_tables(q),) for _, _, sampling, w, h, q, _, _, _, _ in RECORDED]


def test_forward_equals_restatement_in_one_mixed_batch(je, pictures, dev):
    specs = _specs(je)
    assert len({s[2:4] for s in specs}) == 3 and len({s[:2] for s in specs}) == 10  # samplings, sizes and tables mixed
    batch = je.EncodeBatch(specs, dev)
    batch.upload()
    batch.alloc(entropy=False)
    batch.coef.fill_(0x5A5A)
    batch.forward(torch.cat([p.reshape(-1) for p in pictures]))
    torch.cuda.synchronize()
    for i, (case, pic) in enumerate(zip(RECORDED, pictures)):
        header, want = je.torch_jpeg_forward(pic.cpu().numpy(), specs[i][4], *specs[i][2:4])
        got = batch.frame_coef(i).cpu().numpy()
        assert np.array_equal(got, want), case[0]
        assert np.array_equal(got, case[9]), case[0]  # Pillow's coefficients


def test_fused_encode_equals_host_and_pillow_in_one_mixed_batch(je, pictures, host_files):
    qualities = [c[5] for c in RECORDED]
    samplings = [c[2] for c in RECORDED]
    got = je.fused_jpeg_encode(pictures, qualities, samplings)
    for case, g, host in zip(RECORDED, got, host_files):
        assert isinstance(g, bytes), case[0]
        assert g == host, case[0]
        assert g == case[7], case[0]  # Pillow's file with restart_marker_rows=1
    again = je.fused_jpeg_encode(pictures, qualities, samplings)
    assert again == got


def _device_scans(je, dev, sets, capacities=None, guard=0):
    specs = [(h.width, h.height, h.hs[0], h.vs[0], h.quant_array()) for _, h, _ in sets]
    batch = je.EncodeBatch(specs, dev, capacities, guard)
    batch.upload()
    batch.alloc()
    for i, (_, h, coef) in enumerate(sets):
        batch.frame_coef(i).copy_(torch.from_numpy(coef[:h.coef_bytes // 2]))
    batch.entropy()
    torch.cuda.synchronize()
    return batch, batch.scans()


def test_device_entropy_stage_equals_host_on_coefficient_sets(je, jpeg, dev):
    sets = ec.coefficient_sets(jpeg)
    _, scans = _device_scans(je, dev, sets)
    zrl = stuffed = 0
    for (name, h, coef), (data, length, flags) in zip(sets, scans):
        want, stats = je.entropy_encode(h, coef, h.mcus_x)
        assert flags == 0 and length == len(want) and data == want, name
        zrl, stuffed = zrl + stats.zrl, stuffed + stats.stuffed
    assert zrl > 0 and stuffed > 0


def test_fixture_frame_full_size_and_two_copies(je, fixture_frame, dev):
    z = ec.load()
    frame = torch.from_numpy(fixture_frame).to(dev)
    assert tuple(frame.shape) == (900, 1600, 3)  # 57 intervals of 600 blocks
    one = je.fused_jpeg_encode([frame], ec.FIXTURE_QUALITY, "4:2:0")[0]
    assert len(one) == int(z["fixture_length"]) and hashlib.sha256(one).hexdigest() == str(z["fixture_sha256"])
    two = je.fused_jpeg_encode([frame, frame], ec.FIXTURE_QUALITY, "4:2:0")
    assert two[0] == one and two[1] == one


def test_capacity_is_respected_and_reported(je, pictures, host_files, dev):
    names = [c[0] for c in RECORDED]
    pick = [names.index(n) for n in ("420_17x23_q75", "420_700x16_q100", "444_9x7_q100", "420_40x150_q75")]
    frames = [pictures[i] for i in pick]
    scans = [len(host_files[i]) - len(je.stream_headers(_header_of(je, RECORDED[i]), _header_of(je, RECORDED[i]).mcus_x)) for i in pick]
    capacities = [scans[0], scans[1] - 1, scans[2] + 5, scans[3]]  # the second is one byte short
    keep = []
    got = je.fused_jpeg_encode(frames, [RECORDED[i][5] for i in pick], [RECORDED[i][2] for i in pick], capacities, guard=GUARD,
                               _batch_out=keep)
    batch = keep[0]
    result = batch.result.cpu().numpy()
    assert result[:, 1].tolist() == [0, je.FLAG_OVERFLOW, 0, 0]
    assert result[:, 0].tolist() == scans  # the needed length of the frame that did not fit as well
    assert got[1] == (None, scans[1])
    for k in (0, 2, 3):
        assert got[k] == host_files[pick[k]]
    out = batch.out.cpu().numpy()
    for k, d in enumerate(batch.descs):
        end = batch.descs[k + 1].out_off if k + 1 < len(pick) else out.size
        assert end - (d.out_off + d.capacity) >= GUARD
        assert (out[d.out_off + d.capacity:end] == 0xA5).all(), k  # not one byte beyond the capacity
    host_scan = host_files[pick[1]][-scans[1]:]
    d = batch.descs[1]
    assert out[d.out_off:d.out_off + d.capacity].tobytes() == host_scan[:-1]  # what fits is what the stream begins with
    # the dispatcher encodes the short frame once more with the length it reported
    before = dict(je.PATHS)
    retried = je.encode_frames(frames, [RECORDED[i][5] for i in pick], [RECORDED[i][2] for i in pick], capacities)
    assert retried == [host_files[i] for i in pick]
    assert je.PATHS["retried"] == before["retried"] + 1 and je.PATHS["kernel"] == before["kernel"] + 1


def _header_of(je, case):
    from bevfusion_amd import jpeg
    _, _, sampling, w, h, q, _, _, _, _ = case
    qt = je.quant_tables(q)
    return jpeg.make_header(w, h, *je.SAMPLINGS[sampling], [qt[0], qt[1], qt[1]])


def test_bad_descriptors_are_refused_before_any_launch(je, dev):
    from bevfusion_amd import _lib
    lib = _lib.load()
    assert lib.bfhip_jpeg_encode_supported(16, 16, 3, 1) == 0 and lib.bfhip_jpeg_encode_supported(0, 16, 2, 2) == 0
    assert lib.bfhip_jpeg_encode_supported(65536, 16, 2, 2) == 0 and lib.bfhip_jpeg_encode_supported(65535, 1, 2, 2) == 1
    assert lib.bfhip_jpeg_encode_workspace_bytes(16, 16, 3, 1) == 0
    qt = je.quant_tables(75)
    rgb = torch.zeros(16 * 16 * 3, dtype=torch.uint8, device=dev)

    def attempt(mutate=None, null=None, n=None):
        batch = je.EncodeBatch([(16, 16, 2, 2, qt)], dev, guard=GUARD)
        if mutate:
            mutate(batch.descs[0])
        batch.upload()
        batch.alloc()
        batch.result.fill_(-7)
        args = [ctypes.addressof(batch.descs), batch.table.data_ptr(), batch.n if n is None else n, rgb.data_ptr(), rgb.numel(),
                batch.coef.data_ptr(), batch.coef.numel(), batch.workspace.data_ptr(), batch.workspace.numel(), batch.out.data_ptr(),
                batch.out.numel(), batch.result.data_ptr(), _lib.stream_of(rgb)]
        if null is not None:
            args[null] = None
        rc = lib.bfhip_jpeg_encode(*args)
        torch.cuda.synchronize()
        untouched = bool((batch.result == -7).all()) and bool((batch.out == 0xA5).all())
        return rc, untouched

    assert attempt() == (0, False)
    mutations = {
        "zero width": lambda d: setattr(d, "width", 0),
        "zero height": lambda d: setattr(d, "height", 0),
        "width over 65535": lambda d: setattr(d, "width", 65536),
        "sampling 3x1": lambda d: setattr(d, "hs", 3),
        "zero quantisation entry": lambda d: d.quant[1].__setitem__(17, 0),
        "block counts": lambda d: d.block_cols.__setitem__(0, 3),
        "pixels outside": lambda d: setattr(d, "rgb_off", 1),
        "output outside": lambda d: setattr(d, "capacity", 1 << 40),
        "workspace outside": lambda d: setattr(d, "ws_off", 256),
    }
    for name, m in mutations.items():
        rc, untouched = attempt(m)
        assert rc < 0 and untouched, name
    for null in (0, 1, 3, 5, 7, 9, 11):
        rc, untouched = attempt(null=null)
        assert rc < 0 and untouched, null
    rc, untouched = attempt(n=lib.bfhip_jpeg_encode_max_frames() + 1)
    assert rc < 0 and untouched
    rc, untouched = attempt(n=0)
    assert rc < 0 and untouched


def test_end_to_end_render_encode_avi_decode(je, jpeg, dev, tmp_path):
    """render_cameras on the small synthetic sample, encode_frames, MjpegAviWriter; the frames read back from the file are the
    host path's bytes, so they decode to within the host path's own loss, which is printed, not thresholded."""
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    try:
        tool = importlib.import_module("visualize")
    finally:
        sys.path.pop(0)
    from bevfusion_amd import visualize as vz
    path = str(tmp_path / "out.avi")
    mosaics = []
    for meta, frames, points, what in tool.synthetic_samples(2, small=True):
        mosaic, _ = vz.visualize_sample(meta, torch.from_numpy(frames).to(dev), torch.from_numpy(points).to(dev), what,
                                        tool.NUSC_CLASSES, scale=1)
        mosaics.append(mosaic)
    assert mosaics[0].is_cuda and mosaics[0].dtype == torch.uint8
    H, W = mosaics[0].shape[:2]
    before = je.PATHS["kernel"]
    streams = je.encode_frames(mosaics, quality=90)
    assert je.PATHS["kernel"] == before + 1
    with je.MjpegAviWriter(path, 2, W, H) as writer:
        for s in streams:
            writer.write(s)
    back = je.read_avi_frames(path)
    assert len(back) == 2
    for mosaic, got in zip(mosaics, back):
        host = je.encode(mosaic.cpu().numpy(), 90, "4:2:0", 1)
        assert got == host  # the device bytes are the host's: the bound on the decoded difference is the host path's own
        decoded = jpeg.decode(got)
        assert decoded.shape == (H, W, 3)
        print("host path max |decoded - rendered| = %d" % int(np.abs(decoded.astype(np.int32) - mosaic.cpu().numpy().astype(np.int32)).max()))
