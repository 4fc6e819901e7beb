"""CPU: the PNG encoder's specification (bevfusion_amd/png_encode.py) against independent readers -- Pillow, zlib, a chunk walker, a
token reader written from RFC 1951 -- and the plain C++ host path (csrc/png_encode_host.h) against the specification, byte for
byte.  No GPU."""
import io
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import png_encode_cases as pc

ROOT = pc.ROOT
FRAMES = pc.frames()


@pytest.fixture(scope="module")
def pe():
    from bevfusion_amd import png_encode
    return png_encode


@pytest.fixture(scope="module")
def spec_files(pe):
    """The specification's file of every (frame, band_rows), computed once."""
    return {(name, rows): pe.encode(rgb, rows, native=False) for name, rgb in FRAMES.items() for rows in pc.BAND_ROWS}


@pytest.fixture(scope="module")
def fixture_frame():
    return pc.fixture_frame()


@pytest.fixture(scope="module")
def fixture_file(pe, fixture_frame):
    return pe.encode(fixture_frame)


def _idat(png):
    got = pc.chunks(png)
    assert [t for t, _ in got] == [b"IHDR", b"IDAT", b"IEND"]
    return got[0][1], got[1][1]


@pytest.mark.parametrize("rows", pc.BAND_ROWS)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_round_trip(pe, spec_files, name, rows):
    from PIL import Image
    rgb, png = FRAMES[name], spec_files[(name, rows)]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), rgb)
    ihdr, stream = _idat(png)
    assert ihdr == rgb.shape[1].to_bytes(4, "big") + rgb.shape[0].to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])
    assert stream[:2] == b"\x78\x01"
    assert zlib.decompress(stream) == pe.torch_png_filter(rgb).tobytes()
    assert len(stream) - 4 <= pe.default_capacity(rgb.shape[1], rgb.shape[0], rows)


@pytest.mark.parametrize("rows", pc.BAND_ROWS)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_host_path_equals_the_specification(pe, spec_files, name, rows):
    assert pe.encode(FRAMES[name], rows, native=True) == spec_files[(name, rows)]
    assert np.array_equal(pe.host_filter(FRAMES[name]), pe.torch_png_filter(FRAMES[name]))


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_bands_are_independent(pe, name):
    filtered = pe.torch_png_filter(FRAMES[name])
    row = filtered.shape[1]
    for rows in (1, 2, 7):
        stream, offsets = pe.deflate_rle(filtered, row * rows)
        n_bands = -(-filtered.shape[0] // rows)
        assert len(offsets) == n_bands + 1 and offsets[0] == 2 and offsets[-1] == len(stream) - 4
        for b in range(n_bands):
            part = stream[offsets[b]:offsets[b + 1]]
            kind = pc.read_band(stream, offsets[b])
            assert kind[3] == offsets[b + 1] and bool(kind[2]) == (b == n_bands - 1)
            if kind[0] == "dynamic" and b < n_bands - 1:
                assert part[-4:] == b"\x00\x00\xff\xff"
            want = filtered[b * rows:(b + 1) * rows].tobytes()
            assert zlib.decompressobj(-15).decompress(part) == want  # on its own, from the recorded offset


def test_filter_choice_equals_a_loop_restatement(pe):
    rs = np.random.RandomState(3)
    pictures = dict(FRAMES)
    pictures["noise_13x6"] = rs.randint(0, 256, (6, 13, 3)).astype(np.uint8)
    pictures["zero_5x4"] = np.zeros((4, 5, 3), np.uint8)
    tie = np.zeros((3, 4, 3), np.uint8)  # row 1 repeats row 0 shifted by a pixel: Sub and Up cost the same there
    tie[0, :, :] = np.array([10, 20, 30, 40])[:, None]
    tie[1, 1:, :] = tie[0, :-1, :]
    pictures["tie_4x3"] = tie
    for name, rgb in pictures.items():
        got = pe.torch_png_filter(rgb)
        assert got[:, 0].tolist() == pc.loop_filter_types(rgb), name
    flat = pe.torch_png_filter(FRAMES["flat_300x5"])
    assert flat[0, 0] == 1 and flat[1:, 0].tolist() == [2] * 4  # Sub, then Up: both leave zeros, None does not
    zero = pe.torch_png_filter(pictures["zero_5x4"])
    assert zero[:, 0].tolist() == [0] * 4  # every filter leaves zeros: the lowest type
    assert pe.torch_png_filter(FRAMES["hramp_33x9"])[0, 0] == 1 and pe.torch_png_filter(FRAMES["vramp_33x9"])[1:, 0].tolist() == [2] * 8
    assert set(pe.torch_png_filter(FRAMES["smooth_40x40"])[1:, 0].tolist()) <= {3, 4}


def test_a_flat_grey_image_ties_none_and_up_and_takes_none(pe):
    """Value 0 costs nothing under every filter; from row 1 on None and Up tie at zero and the lower type wins."""
    got = pe.torch_png_filter(np.zeros((6, 9, 3), np.uint8))
    assert got[:, 0].tolist() == [0] * 6 and not got.any()


def _kraft(lens):
    return sum(2 ** (15 - v) for v in lens if v)


def _check_lengths(pe, hist):
    lens = pe.huffman_lengths(hist)
    used = [s for s, h in enumerate(hist) if h]
    assert all(0 < lens[s] <= 15 for s in used) and all(lens[s] == 0 for s in range(len(hist)) if not hist[s])
    if len(used) >= 2:
        assert _kraft(lens) == 2 ** 15
    assert sum(h * v for h, v in zip(hist, lens)) <= 9 * sum(hist)
    got = np.zeros(len(hist), np.uint8)
    from bevfusion_amd import _lib
    h32 = np.asarray(hist, np.uint32)
    _lib.call("bfhip_png_huffman_lengths", h32.ctypes.data, len(hist), 15, got.ctypes.data)
    assert got.tolist() == lens  # the C++ the kernels share
    return lens


def test_huffman_lengths(pe):
    rs = np.random.RandomState(5)
    for k in range(40):
        hist = rs.randint(0, [2, 10, 1000, 100000][k % 4], 286) * (rs.rand(286) < [1.0, 0.5, 0.1][k % 3])
        hist[256] = 1
        _check_lengths(pe, [int(h) for h in hist])
    skew = np.zeros(286, np.int64)
    skew[:40] = (1.6 ** np.arange(40)).astype(np.int64) + 1
    _check_lengths(pe, skew.tolist())
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    lens = _check_lengths(pe, fib + [0] * (286 - len(fib)))
    assert max(lens) == 15  # the unlimited tree is 23 deep
    two = [0] * 286
    two[65], two[256] = 1000, 1
    assert _check_lengths(pe, two)[65] == 1 and pe.huffman_lengths(two)[256] == 1
    assert set(_check_lengths(pe, [7] * 286)) == {8, 9}
    assert set(_check_lengths(pe, [7] * 256 + [0] * 30)) == {0, 8}
    one = [0] * 286
    one[256] = 1
    assert pe.huffman_lengths(one)[256] == 1 and sum(pe.huffman_lengths(one)) == 1
    assert pe.huffman_lengths([0] * 286) == [0] * 286
    assert pe.huffman_lengths([5, 1, 1, 3], max_len=2) == [2, 2, 2, 2]
    assert pe.huffman_lengths([8, 1, 1, 2], max_len=3) == [1, 3, 3, 2]  # ties by symbol index do not change an optimal code
    with pytest.raises(ValueError):
        pe.huffman_lengths([1] * 5, max_len=2)


@pytest.mark.parametrize("length", pc.STRETCHES)
def test_run_splitting(pe, length):
    data = pc.stretch_string(length)
    want = pc.expected_tokens(data)
    lit, match = pe.run_tokens(data)
    got = [("lit", int(v)) if m == 0 else ("match", int(m)) for v, m in zip(lit, match)]
    assert got == want
    assert [m for k, m in want if k == "match"] == {1: [], 2: [], 3: [], 4: [3], 258: [257], 259: [258], 260: [258], 261: [258], 517: [258, 258]}[length]
    for native in (False, True):
        stream, offsets = (pe.host_deflate(data, 4096)[:2] if native else pe.deflate_rle(data, 4096))
        assert zlib.decompress(stream) == data and offsets == [2, len(stream) - 4]
        band = pc.read_band(stream, 2)
        if band[0] == "dynamic":  # the tokens in the stream itself
            assert band[1] == want
        else:
            assert length < 258 and band[1] == data
    filler = bytes((i * 5) % 11 for i in range(4000))  # enough cheap literals in front that the band is worth a dynamic block
    stream, _ = pe.deflate_rle(filler + data, 1 << 20)
    band = pc.read_band(stream, 2)
    assert band[0] == "dynamic" and band[1] == pc.expected_tokens(filler + data)


def test_a_stretch_is_cut_at_a_band_boundary(pe):
    data = bytes(range(200)) * 3 + b"Z" * 400 + bytes(range(200))
    cut = 600 + 150
    stream, offsets = pe.deflate_rle(data, cut)
    assert zlib.decompress(stream) == data and len(offsets) == 3
    first, second = pc.read_band(stream, offsets[0]), pc.read_band(stream, offsets[1])
    assert first[0] == second[0] == "dynamic"
    assert first[1] == pc.expected_tokens(data[:cut]) and first[1][-2:] == [("lit", 90), ("match", 149)]
    assert second[1] == pc.expected_tokens(data[cut:]) and second[1][:2] == [("lit", 90), ("match", 249)]
    assert pe.host_deflate(data, cut)[:2] == (stream, offsets)


def test_stored_fallback_and_capacity(pe):
    rs = np.random.RandomState(11)
    noise = rs.randint(0, 256, 70000).astype(np.uint8).tobytes()
    half = noise[:2000] + b"\0" * 2000
    for data, band_bytes, want in ((noise, 70000, [True]), (noise, 4096, [True] * 18), (half, 4000, [False]),
                                   (noise[:4000] + half + noise[:100], 4000, [True, False, True])):
        body, bands = pe.deflate_bands(data, band_bytes)
        assert [b[4] for b in bands] == want
        assert len(body) <= pe.stream_capacity(len(data), band_bytes)
        for b in bands:
            assert b[3] <= pe.stored_bytes(b[2])
        stream, offsets = pe.deflate_rle(data, band_bytes)
        assert zlib.decompress(stream) == data
        got = pe.host_deflate(data, band_bytes)
        assert got[:3] == (stream, offsets, bands)
        assert (got[3].stored_bands, got[3].dynamic_bands, got[3].bytes) == (sum(want), len(want) - sum(want), len(body))
    body, bands = pe.deflate_bands(noise, 70000)
    assert len(body) == 2 + 70000 + 10 == pe.stream_capacity(70000, 70000)  # two stored blocks: the bound is met exactly
    from bevfusion_amd import _lib
    assert _lib.call_size("bfhip_png_capacity", 70000, 4096) == pe.stream_capacity(70000, 4096)
    assert pe.default_capacity(64, 64, 7) == pe.stream_capacity(64 * 193, 7 * 193)
    with pytest.raises(RuntimeError, match="longer than the capacity"):
        pe.host_deflate(noise, 4096, capacity=len(body) - 1000)


def _huffman_cost(hist):
    import heapq
    q = [h for h in hist if h]
    heapq.heapify(q)
    cost = 0
    while len(q) > 1:
        a, b = heapq.heappop(q), heapq.heappop(q)
        cost += a + b
        heapq.heappush(q, a + b)
    return cost


@pytest.mark.parametrize("which", ("fibonacci", "doubling"))
def test_skewed_strings_and_the_length_limit(pe, which):
    data = pc.fibonacci_string() if which == "fibonacci" else pc.doubling_string()
    stream, offsets = pe.deflate_rle(data, len(data))
    band = pc.read_band(stream, 2)
    assert band[0] == "dynamic" and band[1] == [("lit", b) for b in data]
    hist = np.bincount(np.frombuffer(data, np.uint8), minlength=286)
    hist[256] = 1
    cost = sum(int(h) * v for h, v in zip(hist, band[4]))
    if which == "doubling":  # the limit binds: the unlimited code is cheaper and 18 deep
        assert max(band[4]) == 15 and cost > _huffman_cost(hist)
    else:
        assert max(band[4]) <= 15 and cost == _huffman_cost(hist)
    assert zlib.decompress(stream) == data
    assert pe.host_deflate(data, len(data))[:2] == (stream, offsets)


def test_fixture_frame_size_and_round_trip(pe, fixture_frame, fixture_file):
    """At most 1.25 x Pillow's default save of the same pixels: a fixed-code or stored-only encoder lands above 3 x."""
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(fixture_file)).convert("RGB")), fixture_frame)
    buf = io.BytesIO()
    Image.fromarray(fixture_frame).save(buf, format="PNG")
    ratio = len(fixture_file) / len(buf.getvalue())
    print("fixture: %d bytes, Pillow %d, ratio %.4f" % (len(fixture_file), len(buf.getvalue()), ratio))
    assert ratio <= 1.25
    filtered = pe.torch_png_filter(fixture_frame)
    assert np.array_equal(filtered, pe.host_filter(fixture_frame))
    types = np.bincount(filtered[:, 0], minlength=5).tolist()
    assert types == [0, 6, 0, 0, 894]
    _, stream = _idat(fixture_file)
    assert zlib.decompress(stream) == filtered.tobytes()


def test_fixture_frame_host_path_equals_the_specification(pe, fixture_frame, fixture_file):
    assert pe.encode(fixture_frame, native=False) == fixture_file


def test_refusals(pe):
    with pytest.raises(ValueError, match=r"\(4, 4, 3\).*float32"):
        pe.encode_frames([torch.zeros(4, 4, 3)])
    with pytest.raises(ValueError, match=r"\(4, 4, 4\).*uint8"):
        pe.encode_frames([torch.zeros(4, 4, 4, dtype=torch.uint8)])
    with pytest.raises(ValueError, match=r"\(0, 4, 3\)"):
        pe.encode_frames([torch.zeros(0, 4, 3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match=r"\(4, 0, 3\)"):
        pe.encode([np.zeros((4, 0, 3), np.uint8)][0])
    from bevfusion_amd import _lib
    most = _lib.load().bfhip_png_encode_max_frames()
    with pytest.raises(ValueError, match="%d frames" % (most + 1)):
        pe.encode_frames([torch.zeros(1, 1, 3, dtype=torch.uint8)] * (most + 1))
    with pytest.raises(ValueError):
        pe.encode(np.zeros((2, 2, 3), np.uint8), band_rows=0)
    assert _lib.load().bfhip_png_encode_supported(1600, 900, 5) == 1 and _lib.load().bfhip_png_encode_supported(0, 900, 5) == 0
    assert _lib.load().bfhip_png_encode_supported(65535, 65535, 1) == 0  # more than 2^31 filtered bytes


def test_encode_frames_takes_the_host_path_without_a_gpu(pe, tmp_path):
    before = dict(pe.PATHS)
    frames = [torch.from_numpy(FRAMES["half_64x64"]), torch.from_numpy(FRAMES["tiny_2x3"])]
    got = pe.encode_frames(frames, band_rows=7)
    assert got == [pe.encode(f.numpy(), 7, native=False) for f in frames]
    assert pe.PATHS["torch"] == before["torch"] + 1 and pe.PATHS["kernel"] == before["kernel"]
    paths = [str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    pe.write_frames(paths, frames)
    assert [open(p, "rb").read() for p in paths] == pe.encode_frames(frames)


def test_tool_writes_the_same_pixels_through_the_host_path(tmp_path):
    from PIL import Image
    tool = os.path.join(ROOT, "tools", "visualize.py")
    for enc in ("pillow", "device"):
        r = subprocess.run([sys.executable, tool, "--synthetic", "--small", "--frames", "2", "--device", "cpu", "--png-encoder", enc,
                            "--out", str(tmp_path / enc)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert "png: host path" in r.stdout
    for sub in ("cameras", "bev"):
        for k in range(2):
            a = np.asarray(Image.open(str(tmp_path / "pillow" / sub / ("%06d.png" % k))))
            b = np.asarray(Image.open(str(tmp_path / "device" / sub / ("%06d.png" % k))))
            assert a.shape == b.shape and a.ndim == 3 and np.array_equal(a, b)


def test_host_code_under_sanitisers(tmp_path, pe):
    """tools/png_encode_host_check.cpp (its own main, the header included) built with AddressSanitizer and UBSan, run as a child
    process over byte strings and frames through exactly-sized and too-small heap blocks."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitiser runtime")
    exe = tmp_path / "png_encode_host_check"
    r = subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "png_encode_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines, want = [], {}
    rs = np.random.RandomState(2)
    strings = {"fib": (pc.fibonacci_string(), 1 << 20), "doubling": (pc.doubling_string(), 1 << 20), "noise": (rs.randint(0, 256, 70000).astype(np.uint8).tobytes(), 66000),
               "runs": (b"".join(pc.stretch_string(k) for k in pc.STRETCHES) * 3, 700), "one": (b"x", 1)}
    for name, (data, band_bytes) in strings.items():
        p = tmp_path / (name + ".bin")
        p.write_bytes(data)
        lines.append("D %s %d" % (p, band_bytes))
        want[str(p)] = pe.deflate_rle(data, band_bytes)[0][:-4]
    for name in ("tiny_1x1", "flat_87x2", "half_64x64", "smooth_40x40"):
        rgb = FRAMES[name]
        p = tmp_path / (name + ".rgb")
        p.write_bytes(rgb.tobytes())
        lines.append("F %s %d %d" % (p, rgb.shape[1], rgb.shape[0]))
        want[str(p)] = pe.torch_png_filter(rgb).tobytes()
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(manifest), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "strings 5 frames 4" in r.stdout
    for path, data in want.items():
        assert open(path + ".out", "rb").read() == data, path
