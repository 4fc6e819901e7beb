"""CPU: the host half of the JPEG decoder (csrc/jpeg_host.h through bfhip_jpeg_parse / bfhip_jpeg_entropy_decode) followed by
the restatement of the device half (jpeg.torch_jpeg_decode) equals Pillow's decode bit for bit; malformed bytes are refused or
decoded without a byte written outside the buffer."""
import ctypes
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
STREAMS = jc.streams()
GUARD = 64


@pytest.fixture(scope="module")
def jpeg():
    import bevfusion_amd
    from bevfusion_amd import _lib, jpeg
    if not os.path.exists(_lib.LIB_PATH):
        bevfusion_amd.build()
    return jpeg


def test_recorded_cases_are_the_issue_s():
    names = [n for n, _, _ in STREAMS]
    for sub, sizes in jc.SIZES.items():
        for (w, h) in sizes:
            for q in jc.QUALITIES:
                assert "%s_%dx%d_q%d" % (jc.SAMPLING_NAME[sub], w, h, q) in names
    assert any(n.endswith("optimize") for n in names) and any(n.endswith("restart") for n in names)
    restart = dict((n, b) for n, b, _ in STREAMS)["420_17x23_q75_restart"]
    assert b"\xff\xdd" in restart


@pytest.mark.parametrize("name,data,pixels", STREAMS, ids=[s[0] for s in STREAMS])
def test_synthetic_stream_equals_pillow(jpeg, name, data, pixels):
    header = jpeg.parse(data)
    assert header.supported == 1, jpeg.REASONS.get(header.reason)
    assert (header.height, header.width) == pixels.shape[:2]
    if name.endswith("restart"):
        assert header.restart_interval > 0
    got = jpeg.decode(data)
    assert got.dtype == np.uint8 and np.array_equal(got, pixels)


def test_header_geometry(jpeg):
    data = dict((n, b) for n, b, _ in STREAMS)["420_17x23_q75"]
    h = jpeg.parse(data)
    assert (h.width, h.height, h.ncomp) == (17, 23, 3)
    assert list(h.hs) == [2, 1, 1] and list(h.vs) == [2, 1, 1]
    assert (h.mcus_x, h.mcus_y) == (2, 2)
    assert list(h.block_cols) == [4, 2, 2] and list(h.block_rows) == [4, 2, 2]
    assert list(h.coef_offset) == [0, 16 * 64, 20 * 64] and h.coef_bytes == 24 * 64 * 2
    q = h.quant_array()
    assert q.dtype == np.uint16 and q.min() >= 1 and q.max() <= 255
    assert q[0, 0] <= q[0, 63]  # natural order: the DC step is the finest of Pillow's tables


def test_fixture_frame_equals_recorded_pillow_decode(jpeg):
    z = jc.load()
    data = open(jc.FIXTURE, "rb").read()
    assert len(data) == 131197
    header = jpeg.parse(data)
    assert header.supported == 1
    H, W = (int(v) for v in z["fixture_shape"])
    assert (header.height, header.width) == (H, W) == (900, 1600)
    assert header.block_rows[0] * 8 > H  # the bottom MCU row is partial
    got = jpeg.decode(data)
    assert got.shape == (H, W, 3)
    assert np.array_equal(got[:32, :32], z["fixture_window_top_left"])
    assert np.array_equal(got[H - 32:, W - 32:], z["fixture_window_bottom_right"])
    assert np.array_equal(got[H // 2 - 16:H // 2 + 16, W // 2 - 16:W // 2 + 16], z["fixture_window_centre"])
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(z["fixture_sha256"])


def test_random_streams_equal_pillow(jpeg):
    pytest.importorskip("PIL")
    specs = jc.random_specs()
    assert len(specs) >= 36
    for seed, w, h, sub, q, kw in specs:
        data = jc.encode(jc.picture(seed, w, h), q, sub, **kw)
        header = jpeg.parse(data)
        assert header.supported == 1, (w, h, sub, q, jpeg.REASONS.get(header.reason))
        assert np.array_equal(jpeg.decode(data), jc.pillow_decode(data)), (seed, w, h, sub, q, kw)


def test_unsupported_streams_say_so(jpeg):
    reasons = {}
    for name, data in jc.unsupported_streams():
        h = jpeg.parse(data)
        assert h.supported == 0 and not jpeg.supported(data)
        reasons[name] = h.reason
        with pytest.raises(RuntimeError):
            jpeg.entropy_decode(data)
    assert reasons == {"progressive": 1, "grayscale": 4}


def _guarded_decode(lib, data, header, coef_bytes):
    """bfhip_jpeg_entropy_decode into a buffer of coef_bytes with GUARD bytes of 0xA5 on either side: (rc, guards intact)."""
    buf = np.full(coef_bytes + 2 * GUARD, 0xA5, np.uint8)
    arr = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    rc = lib.bfhip_jpeg_entropy_decode(arr.ctypes.data, len(data), ctypes.addressof(header), buf.ctypes.data + GUARD, coef_bytes)
    return rc, bool((buf[:GUARD] == 0xA5).all() and (buf[GUARD + coef_bytes:] == 0xA5).all())


@pytest.mark.parametrize("name,data,pixels", STREAMS, ids=[s[0] for s in STREAMS])
def test_malformed_input_is_refused_or_decoded_inside_the_buffer(jpeg, name, data, pixels):
    from bevfusion_amd import _lib
    lib = _lib.load()
    good = jpeg.parse(data)
    rc, intact = _guarded_decode(lib, data, good, good.coef_bytes)
    assert rc == 0 and intact
    rc, intact = _guarded_decode(lib, data, good, good.coef_bytes - 2)  # too small
    assert rc < 0 and intact and b"too small" in lib.bfhip_last_error()
    outcomes = set()
    for k, bad in enumerate(jc.malformed(data, seed=len(data))):
        arr = np.frombuffer(bad, np.uint8) if len(bad) else np.zeros(1, np.uint8)
        h = jpeg.Header()
        rc = lib.bfhip_jpeg_parse(arr.ctypes.data, len(bad), ctypes.addressof(h))
        assert rc <= 0
        if rc < 0 or not h.supported or h.coef_bytes > (1 << 24):
            outcomes.add("refused")
            # the entropy stage parses again and must refuse as well, whatever header it is handed
            rc, intact = _guarded_decode(lib, bad, good, good.coef_bytes)
            assert intact and (rc < 0 or k >= 16)  # a corrupted byte may sit where the scan does not care
            continue
        rc, intact = _guarded_decode(lib, bad, h, h.coef_bytes)
        assert rc <= 0 and intact
        outcomes.add("decoded" if rc == 0 else "refused")
    assert "refused" in outcomes


def test_truncated_scan_zero_fills_the_rest(jpeg):
    """An EOI reached early: the blocks behind the point where the data ended are zero (libjpeg's premature-end path)."""
    data = dict((n, b) for n, b, _ in STREAMS)["420_33x9_q100"]
    header, full = jpeg.entropy_decode(data)
    cut = data[:len(data) - (len(data) - data.index(b"\xff\xda")) // 2]
    h2, part = jpeg.entropy_decode(cut)
    assert h2.coef_bytes == header.coef_bytes
    assert np.array_equal(part[:64], full[:64])  # the first block came before the cut
    last_cr = part[header.coef_offset[2]:].reshape(-1, 64)[-1]
    assert not last_cr.any() and full[header.coef_offset[2]:].reshape(-1, 64)[-1].any()


def test_wraparound_is_defined_on_full_range_coefficients(jpeg):
    """torch_jpeg_decode on int16 extremes: no error, no warning, deterministic."""
    rs = np.random.RandomState(3)
    q = rs.randint(1, 256, (3, 64))
    header = jpeg.make_header(17, 23, 2, 2, q)
    coef = rs.randint(-32768, 32768, header.coef_bytes // 2).astype(np.int16)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a = jpeg.torch_jpeg_decode(header, coef)
        b = jpeg.torch_jpeg_decode(header, coef.copy())
    assert a.shape == (23, 17, 3) and a.dtype.is_floating_point is False and bool((a == b).all())


def test_host_decoder_under_sanitisers(tmp_path):
    """tools/jpeg_host_check.cpp (its own main, the header included) built with AddressSanitizer and UBSan, run as a child
    process over every recorded stream, its truncations and corruptions and the unsupported streams."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitiser runtime")
    exe = tmp_path / "jpeg_host_check"
    r = subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "jpeg_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    paths = []
    for name, data, _ in STREAMS:
        for k, variant in enumerate([data] + jc.malformed(data, seed=len(data))):
            p = tmp_path / ("%s_%02d.jpg" % (name, k))
            p.write_bytes(variant)
            paths.append(str(p))
    for name, data in jc.unsupported_streams():
        p = tmp_path / ("unsupported_%s.jpg" % name)
        p.write_bytes(data)
        paths.append(str(p))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(paths) + "\n")
    r = subprocess.run([str(exe), str(manifest)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = dict(zip(r.stdout.split()[0::2], map(int, r.stdout.split()[1::2])))
    assert counts["files"] == len(paths) and counts["decoded"] >= len(STREAMS) and counts["malformed"] > 0
    assert counts["refused"] >= counts["decoded"]
