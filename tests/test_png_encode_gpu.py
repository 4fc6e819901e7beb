"""GPU: the device path of the PNG encoder (csrc/png_encode.hip) against the host path (csrc/png_encode_host.h), byte for byte;
tests/test_png_encode_cpu.py holds the host path to the specification and to Pillow and zlib."""
import hashlib
import io
import zlib

import numpy as np
import pytest
import torch

import png_encode_cases as pc

pytestmark = pytest.mark.gpu

FRAMES = pc.frames()
JOBS = [(name, rows) for name in sorted(FRAMES) for rows in pc.BAND_ROWS]
GUARD, FILL = 64, 0x5A
FIXTURE_SHA256 = "1856fb1f092df21e6d02a3c1d24ca6a642e40916eb2d2f288cddfef3473b3f01"


@pytest.fixture(scope="module")
def pe():
    from bevfusion_amd import png_encode
    return png_encode


@pytest.fixture(scope="module")
def mixed(pe, dev):
    """Every frame at every band size in ONE batch, the workspace and the output filled with 0x5A first: (files, batch)."""
    keep = []
    files = pe.fused_png_encode([torch.from_numpy(FRAMES[name]).to(dev) for name, _ in JOBS], [rows for _, rows in JOBS], guard=GUARD,
                                fill=FILL, _batch_out=keep)
    return files, keep[0]


@pytest.fixture(scope="module")
def host_files(pe):
    return [pe.encode(FRAMES[name], rows) for name, rows in JOBS]


@pytest.mark.parametrize("k", range(len(JOBS)), ids=["%s-%s" % j for j in JOBS])
def test_mixed_batch_equals_the_host_path(mixed, host_files, k):
    assert mixed[0][k] == host_files[k]


def test_mixed_batch_mixes_and_decodes(pe, mixed):
    from PIL import Image
    files, batch = mixed
    got = batch.streams()
    kinds = {(name, rows): [b[4] for b in bands] for (name, rows), (_, _, _, bands, _) in zip(JOBS, got)}
    assert all(kinds[("noise_64x64", rows)] == [True] * len(kinds[("noise_64x64", rows)]) for rows in pc.BAND_ROWS)  # stored
    assert kinds[("half_64x64", None)] == [False] and kinds[("flat_300x5", 1)] == [False] * 5                      # dynamic
    assert len(kinds[("half_64x64", 7)]) == 10 and len({d.n_bytes for d in batch.descs}) >= 9                       # many bands, many sizes
    for (name, _), png in zip(JOBS, files):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), FRAMES[name])


def test_nothing_is_written_past_a_stream(mixed):
    """Behind every stream the 0x5A the buffer was filled with: up to the capacity, and in the guard beyond it."""
    _, batch = mixed
    out = batch.out.cpu().numpy()
    got = batch.streams()
    ends = [d.out_off for d in batch.descs][1:] + [out.size]
    for d, (_, length, flags, _, _), end in zip(batch.descs, got, ends):
        assert flags == 0 and 2 < length <= d.capacity
        assert end - (d.out_off + d.capacity) >= GUARD
        assert (out[d.out_off + length:end] == FILL).all()


def test_a_smaller_capacity_is_reported_and_respected(pe, dev):
    frames = [torch.from_numpy(FRAMES[n]).to(dev) for n in ("noise_64x64", "half_64x64", "smooth_40x40")]
    keep = []
    full = pe.fused_png_encode(frames, 7)
    got = pe.fused_png_encode(frames, 7, capacity=[None, 1000, None], guard=GUARD, fill=FILL, _batch_out=keep)
    assert got[0] == full[0] and got[2] == full[2]
    assert got[1][0] is None and got[1][1] == len(pc.chunks(full[1])[1][1]) - 4  # the needed length, without the Adler-32
    batch = keep[0]
    out = batch.out.cpu().numpy()
    d = batch.descs[1]
    assert (out[d.out_off + 1000:batch.descs[2].out_off] == FILL).all()
    assert out[d.out_off:d.out_off + 1000].tobytes() == pc.chunks(full[1])[1][1][:1000]


def test_device_deflate(pe, dev):
    rs = np.random.RandomState(11)
    filler = bytes((i * 5) % 11 for i in range(4000))
    noise = rs.randint(0, 256, 70000).astype(np.uint8).tobytes()
    jobs = [(pc.fibonacci_string(), 1 << 20), (pc.doubling_string(), 1 << 20), (noise, 70000), (noise, 4096),
            (noise[:4000] + noise[:2000] + b"\0" * 2000 + noise[:100], 4000), (b"x", 1), (b"\0" * 70000, 1 << 20),
            (bytes(range(200)) * 3 + b"Z" * 400 + bytes(range(200)), 750)]
    for k in pc.STRETCHES:
        jobs += [(pc.stretch_string(k), 4096), (filler + pc.stretch_string(k), 1 << 20), (pc.stretch_string(k) * 40, 97)]
    keep = []
    got = pe.fused_deflate([torch.from_numpy(np.frombuffer(d, np.uint8).copy()).to(dev) for d, _ in jobs], [b for _, b in jobs],
                           guard=GUARD, fill=FILL, _batch_out=keep)
    for (data, band_bytes), (stream, offsets, bands) in zip(jobs, got):
        want = pe.host_deflate(data, band_bytes)
        assert (stream, offsets, bands) == want[:3], (len(data), band_bytes)
        assert zlib.decompress(stream) == data
    heads = [h for _, _, _, _, h in keep[0].streams()]
    assert heads[1][5] == 15 and heads[1][4] == 1             # the doubling string: one dynamic band, its longest code 15 bits
    assert heads[2][3] == 1 and heads[3][3] == 18             # noise: stored, whole or in 18 bands
    assert (heads[4][3], heads[4][4]) == (2, 1)               # stored, dynamic, stored
    out = keep[0].out.cpu().numpy()
    ends = [d.out_off for d in keep[0].descs][1:] + [out.size]
    for d, (_, length, _, _, _), end in zip(keep[0].descs, keep[0].streams(), ends):
        assert (out[d.out_off + length:end] == FILL).all()


def test_fixture_frame(pe, dev):
    frame = pc.fixture_frame()
    got = pe.fused_png_encode([torch.from_numpy(frame).to(dev)])[0]
    assert got == pe.encode(frame)
    assert hashlib.sha256(got).hexdigest() == FIXTURE_SHA256


def test_switch_takes_the_host_path_with_the_same_bytes(pe, dev, monkeypatch):
    frames = [torch.from_numpy(FRAMES[n]).to(dev) for n in ("half_64x64", "tiny_2x3", "smooth_40x40")]
    before = dict(pe.PATHS)
    on = pe.encode_frames(frames, 7)
    assert pe.PATHS["kernel"] == before["kernel"] + 1 and pe.PATHS["torch"] == before["torch"]
    monkeypatch.setattr(pe, "ENABLED", False)  # what BFHIP_PNG_ENCODE=0 sets at import
    off = pe.encode_frames(frames, 7)
    assert pe.PATHS["kernel"] == before["kernel"] + 1 and pe.PATHS["torch"] == before["torch"] + 1
    assert on == off


def test_the_batch_takes_four_launches_and_one_read(pe):
    """Structure, not timing: the entry point's launch list is fixed in csrc/png_encode.hip (png_launch) whatever the batch."""
    import os
    src = open(os.path.join(pc.ROOT, "bevfusion-3d_object_detection_amd", "csrc", "png_encode.hip")).read()
    body = src[src.index("static int png_launch"):src.index("static int png_run")]
    assert body.count("hipLaunchKernelGGL") == 4 and "for (" not in body
