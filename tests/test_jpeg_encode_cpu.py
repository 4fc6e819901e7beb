"""CPU: the JPEG encoder's specification (jpeg_encode.quant_tables, torch_jpeg_forward, build_stream over the host entropy
encoder csrc/jpeg_encode_host.h) gives Pillow's quantisation tables, Pillow's coefficients and Pillow's file, bit for bit and
byte for byte, on the recorded cases of tests/golden/jpeg_encode_cases.npz; the entropy stage round-trips through the package's
decoder on hand-made and seeded coefficients and refuses what it cannot code; the AVI writer's file is walked by a RIFF reader
of the test's own."""
import ctypes
import hashlib
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_encode_cases as ec

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RECORDED = ec.recorded()
IDS = [c[0] for c in RECORDED]
GUARD = 64


@pytest.fixture(scope="module")
def je():
    import bevfusion_amd
    from bevfusion_amd import _lib, jpeg_encode
    if not os.path.exists(_lib.LIB_PATH):
        bevfusion_amd.build()
    return jpeg_encode


@pytest.fixture(scope="module")
def jpeg(je):
    from bevfusion_amd import jpeg
    return jpeg


@pytest.fixture(scope="module")
def sets(jpeg):
    return ec.coefficient_sets(jpeg)


def test_recorded_cases_are_the_issue_s():
    assert len(RECORDED) == 24
    for name in ("420_1x1_q30", "420_16x16_q75", "420_17x23_q100", "420_33x9_q30", "420_22x31_q75", "420_40x150_q75",
                 "420_700x16_q100", "420_64x64_q5", "422_19x10_q100", "444_9x7_q30"):
        assert name in IDS
    assert os.path.getsize(ec.NPZ) < 200 * 1024


@pytest.mark.parametrize("q", ec.QUANT_QUALITIES)
def test_quant_tables_equal_pillow(je, jpeg, q):
    want = jpeg.parse(ec.load()["quant_q%d_file" % q].tobytes()).quant_array()
    got = je.quant_tables(q)
    assert got.dtype == np.uint16 and got.shape == (2, 64)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[1], want[2])


@pytest.mark.parametrize("case", RECORDED, ids=IDS)
def test_forward_equals_pillow_coefficients(je, jpeg, case):
    name, seed, sampling, w, h, q, noise, rows1, _, coef = case
    header, got = je.torch_jpeg_forward(ec.pixels(seed, w, h, noise), je.quant_tables(q), *je.SAMPLINGS[sampling])
    want = jpeg.parse(rows1)
    assert got.dtype == np.int16 and header.coef_bytes == want.coef_bytes
    assert list(header.block_cols) == list(want.block_cols) and list(header.coef_offset) == list(want.coef_offset)
    assert np.array_equal(header.quant_array(), want.quant_array())
    assert np.array_equal(got, coef)
    # the decoder's layout: the package's own decoder takes it
    assert np.array_equal(jpeg.torch_jpeg_decode(header, got).numpy(), jpeg.decode(rows1))


def test_forward_equals_pillow_on_random_specs(je, jpeg):
    pytest.importorskip("PIL")
    specs = jc.random_specs()
    assert len(specs) == 42
    for seed, w, h, sub, q, _ in specs:
        px = jc.picture(seed, w, h)
        _, want = jpeg.entropy_decode(jc.encode(px, q, sub))
        _, got = je.torch_jpeg_forward(px, je.quant_tables(q), *je.SAMPLINGS[{0: "4:4:4", 1: "4:2:2", 2: "4:2:0"}[sub]])
        assert np.array_equal(got, want), (seed, w, h, sub, q)


@pytest.mark.parametrize("case", RECORDED, ids=IDS)
def test_stream_is_pillow_s_file(je, jpeg, case):
    name, seed, sampling, w, h, q, noise, rows1, rows0, _ = case
    px = ec.pixels(seed, w, h, noise)
    assert je.encode(px, q, sampling, 1) == rows1
    assert je.encode(px, q, sampling, 0) == rows0
    assert b"\xff\xdd" in rows1 and b"\xff\xdd" not in rows0[:rows0.index(b"\xff\xda")]


def test_cases_exercise_what_they_claim(je, jpeg):
    by_name = {c[0]: c for c in RECORDED}
    header, coef = jpeg.entropy_decode(by_name["420_700x16_q100"][7])
    _, stats = je.entropy_encode(header, coef, header.mcus_x)
    # uniform RGB noise at q100 reaches category 8 (|x| < 256) and no further; categories 9 to 11 are the coefficient sets'
    assert header.mcus_x * 6 == 264 and stats.stuffed > 100 and stats.max_ac_category == 8 and stats.max_dc_category >= 8
    wraps = by_name["420_40x150_q75"][7]
    header = jpeg.parse(wraps)
    assert header.mcus_y == 10 and header.restart_interval == header.mcus_x
    scan = wraps[wraps.index(b"\xff\xda"):]
    assert [scan.count(bytes([0xFF, 0xD0 + m])) for m in range(8)] == [2, 1, 1, 1, 1, 1, 1, 1]  # D0..D7, then D0 again
    header, coef = jpeg.entropy_decode(by_name["420_64x64_q5"][7])
    _, stats = je.entropy_encode(header, coef, header.mcus_x)
    assert stats.zrl == 0 and stats.eob == 96 and (coef.reshape(-1, 64)[:, 1:] != 0).any(1).sum() <= 10  # of 96 blocks
    header, coef = jpeg.entropy_decode(by_name["420_1x1_q75"][7])
    luma = coef[:4 * 64].reshape(4, 64)
    assert not luma[1:, 1:].any() and (luma[1:, 0] == luma[0, 0]).all()  # three dummies with the real block's DC


def test_fixture_frame_length_and_sha256(je, jpeg):
    z = ec.load()
    frame = jpeg.decode(open(jc.FIXTURE, "rb").read())
    data = je.encode(frame, ec.FIXTURE_QUALITY, "4:2:0", 1)
    assert len(data) == int(z["fixture_length"])
    assert hashlib.sha256(data).hexdigest() == str(z["fixture_sha256"])


def test_pillow_decodes_our_bytes_as_its_own(je):
    Image = pytest.importorskip("PIL.Image")
    for name, seed, sampling, w, h, q, noise, rows1, _, _ in RECORDED:
        ours = je.encode(ec.pixels(seed, w, h, noise), q, sampling, 1)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(ours)).convert("RGB")), jc.pillow_decode(rows1)), name


def test_entropy_stage_round_trips_on_coefficient_sets(je, jpeg, sets):
    zrl = stuffed = 0
    ac = dc = 0
    for name, header, coef in sets:
        for rows in (1, 0):
            data = je.build_stream(header, coef, rows)
            parsed, back = jpeg.entropy_decode(data)
            assert parsed.supported and np.array_equal(back, coef), (name, rows)
        _, stats = je.entropy_encode(header, coef, header.mcus_x)
        zrl, stuffed = zrl + stats.zrl, stuffed + stats.stuffed
        ac, dc = max(ac, stats.max_ac_category), max(dc, stats.max_dc_category)
    assert zrl > 0 and stuffed > 0 and ac == 10 and dc == 11
    by_name = {n: (h, c) for n, h, c in sets}
    scan, stats = je.entropy_encode(*by_name["byte_aligned"], 1)
    assert scan == b"\x5a\x00\xff\xd9" and stats.bytes == 4  # 16 bits and no padding
    _, stats = je.entropy_encode(*by_name["runs"], 0)
    assert stats.zrl >= 3 * 7 and stats.eob < 3 * 12  # blocks whose coefficient 63 is set end without an EOB
    _, stats = je.entropy_encode(*by_name["dc_steps"], 0)
    assert stats.max_dc_category == 11


def _guarded_encode(je, header, coef, interval, capacity):
    from bevfusion_amd import _lib
    lib = _lib.load()
    buf = np.full(capacity + 2 * GUARD, 0xA5, np.uint8)
    stats = je.Stats()
    rc = lib.bfhip_jpeg_entropy_encode(ctypes.addressof(header), coef.ctypes.data, coef.nbytes, interval, buf.ctypes.data + GUARD,
                                       capacity, ctypes.addressof(stats))
    intact = bool((buf[:GUARD] == 0xA5).all() and (buf[GUARD + capacity:] == 0xA5).all())
    return rc, intact, stats, buf[GUARD:GUARD + capacity], lib.bfhip_last_error()


def test_refusals(je, jpeg, sets):
    by_name = {n: (h, c) for n, h, c in sets}
    header, coef = by_name["random_420"]
    want, _ = je.entropy_encode(header, coef, header.mcus_x)
    rc, intact, stats, got, _ = _guarded_encode(je, header, coef, header.mcus_x, len(want))
    assert rc == 0 and intact and got.tobytes() == want
    rc, intact, stats, got, msg = _guarded_encode(je, header, coef, header.mcus_x, len(want) - 1)  # one byte short
    assert rc < 0 and intact and stats.bytes == len(want) and b"too small" in msg
    assert got.tobytes() == want[:-1]
    bad = coef.copy()
    bad[header.coef_offset[1] + 64 + 5] = 1024  # an AC coefficient
    rc, intact, _, _, msg = _guarded_encode(je, header, bad, header.mcus_x, len(want) + 64)
    assert rc < 0 and intact and b"AC coefficient" in msg
    bad[header.coef_offset[1] + 64 + 5] = -1024
    assert _guarded_encode(je, header, bad, header.mcus_x, len(want) + 64)[0] < 0
    h2, c2 = by_name["dc_steps"]
    bad = c2.copy()
    bad[64] = bad[0] + 2048  # a DC difference
    rc, intact, _, _, msg = _guarded_encode(je, h2, bad, 0, 4096)
    assert rc < 0 and intact and b"DC difference" in msg
    bad[64] = bad[0] + 2047
    assert _guarded_encode(je, h2, bad, 0, 4096)[0] == 0
    wrong = jpeg.make_header(40, 37, 2, 2, np.ones((3, 64)))
    wrong.block_cols[0] += 1  # block counts that do not fit the size
    rc, intact, _, _, msg = _guarded_encode(je, wrong, coef, header.mcus_x, len(want) + 64)
    assert rc < 0 and intact and b"block counts" in msg
    with pytest.raises(RuntimeError):
        je.entropy_encode(header, coef[:-64], header.mcus_x)  # fewer coefficients than the header names


def test_host_encoder_under_sanitisers(tmp_path, jpeg, sets):
    """tools/jpeg_encode_host_check.cpp (its own main, the header included) built with AddressSanitizer and UBSan, run as a
    child process over the coefficient sets through exactly-sized and too-small heap blocks."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitiser runtime")
    exe = tmp_path / "jpeg_encode_host_check"
    r = subprocess.run([cxx] + flags + [os.path.join(ROOT, "tools", "jpeg_encode_host_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = []
    for name, header, coef in sets:
        p = tmp_path / (name + ".i16")
        coef[:header.coef_bytes // 2].tofile(str(p))
        lines.append("%s %d %d %d %d" % (p, header.width, header.height, header.hs[0], header.vs[0]))
    header, coef = {n: (h, c) for n, h, c in sets}["random_422"]
    illegal = coef.copy()
    illegal[64 * 3 + 9] = -1024
    p = tmp_path / "illegal.i16"
    illegal.tofile(str(p))
    lines.append("%s %d %d %d %d" % (p, header.width, header.height, header.hs[0], header.vs[0]))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(manifest)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = dict(zip(r.stdout.split()[0::2], map(int, r.stdout.split()[1::2])))
    assert counts == {"sets": len(sets) + 1, "encoded": 3 * len(sets), "refused": 6 * len(sets) + len(sets) + 1, "illegal": 3}


# ---------------------------------------------------------------------------------------------- AVI
def _riff_chunks(blob, begin, end):
    """[(tag, list type or None, payload begin, payload size)] of the chunks in blob[begin:end]."""
    out, p = [], begin
    while p < end:
        tag, size = blob[p:p + 4], struct.unpack_from("<I", blob, p + 4)[0]
        assert p + 8 + size <= end, "chunk %r runs past its parent" % tag
        out.append((tag, blob[p + 8:p + 12] if tag in (b"RIFF", b"LIST") else None, p + 8, size))
        p += 8 + size + (size & 1)
    assert p == end or p == end + 1
    return out


def test_avi_file_walked_by_an_independent_reader(je, tmp_path):
    pool = [je.encode(jc.picture(k, 24, 16) if k % 2 else ec.pixels(k, 24, 16, True), 90 - 4 * k, "4:2:0", 1) for k in range(16)]
    odd, even = [f for f in pool if len(f) & 1], [f for f in pool if not len(f) & 1]
    assert odd and even  # a chunk that needs its padding byte and one that does not
    frames = [even[0], odd[0], (odd + even)[-1]]
    path = str(tmp_path / "t.avi")
    with je.MjpegAviWriter(path, 2, 24, 16) as w:
        for f in frames:
            w.write(f)
        with pytest.raises(ValueError):
            w.write(je.encode(jc.picture(9, 16, 16), 90, "4:2:0", 1))  # another size
    blob = open(path, "rb").read()
    (tag, kind, at, size), = _riff_chunks(blob, 0, len(blob))
    assert (tag, kind) == (b"RIFF", b"AVI ") and size == len(blob) - 8
    top = _riff_chunks(blob, at + 4, at + size)
    assert [(t, k) for t, k, _, _ in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl = _riff_chunks(blob, top[0][2] + 4, top[0][2] + top[0][3])
    assert [(t, k) for t, k, _, _ in hdrl] == [(b"avih", None), (b"LIST", b"strl")]
    avih = struct.unpack_from("<14I", blob, hdrl[0][2])
    assert hdrl[0][3] == 56 and avih[0] == 500000 and avih[3] & 0x10 and avih[4] == 3 and avih[6] == 1 and avih[8:10] == (24, 16)
    assert avih[7] == max(len(f) for f in frames)
    strl = _riff_chunks(blob, hdrl[1][2] + 4, hdrl[1][2] + hdrl[1][3])
    assert [t for t, _, _, _ in strl] == [b"strh", b"strf"]
    strh = struct.unpack_from("<4s4sIHHIIIIIIII4H", blob, strl[0][2])
    assert strl[0][3] == 56 and strh[:2] == (b"vids", b"MJPG") and strh[7] / strh[6] == 2.0 and strh[9] == 3 and strh[-2:] == (24, 16)
    strf = struct.unpack_from("<IiiHH4sIiiII", blob, strl[1][2])
    assert strl[1][3] == 40 and strf[:6] == (40, 24, 16, 1, 24, b"MJPG")
    movi_at = top[1][2]  # of the 'movi' tag
    chunks = _riff_chunks(blob, movi_at + 4, movi_at + top[1][3])
    assert [t for t, _, _, _ in chunks] == [b"00dc"] * 3
    for (_, _, begin, n), f in zip(chunks, frames):
        assert (begin - 8) % 2 == 0 and blob[begin:begin + n] == f
    index = [struct.unpack_from("<4sIII", blob, top[2][2] + 16 * k) for k in range(3)]
    assert top[2][3] == 48
    for (tag, flags, off, n), (_, _, begin, size) in zip(index, chunks):
        assert tag == b"00dc" and flags & 0x10 and movi_at + off == begin - 8 and n == size
        assert blob[movi_at + off:movi_at + off + 4] == b"00dc" and struct.unpack_from("<I", blob, movi_at + off + 4)[0] == n
    assert je.read_avi_frames(path) == frames


def test_avi_refuses_a_file_past_the_riff_limit(je, tmp_path, monkeypatch):
    frame = je.encode(jc.picture(1, 16, 16), 75, "4:2:0", 1)
    monkeypatch.setattr(je, "AVI_LIMIT", 4096)
    w = je.MjpegAviWriter(str(tmp_path / "big.avi"), 2, 16, 16)
    with pytest.raises(ValueError, match="AVI 1.0"):
        for _ in range(16):
            w.write(frame)
    w.close()
    assert len(je.read_avi_frames(str(tmp_path / "big.avi"))) >= 1 and os.path.getsize(str(tmp_path / "big.avi")) <= 4096


def test_dispatcher_takes_the_host_path_without_a_gpu(je):
    import torch
    px = jc.picture(5, 17, 23)
    before = je.PATHS["torch"]
    got = je.encode_frames([torch.from_numpy(px)], 75, "4:2:0")
    assert je.PATHS["torch"] == before + 1 and got == [je.encode(px, 75, "4:2:0", 1)]


def test_tool_writes_a_video_of_the_rendered_frames(je, jpeg, tmp_path):
    """tools/visualize.py --video on the host path: the AVI's frames are the encoder's bytes of the PNG frames beside them."""
    Image = pytest.importorskip("PIL.Image")
    import sys
    out = str(tmp_path / "vis")
    video = str(tmp_path / "cams.avi")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "visualize.py"), "--synthetic", "--small", "--frames", "2", "--scale",
                        "2", "--device", "cpu", "--out", out, "--video", video, "--quality", "80"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    back = je.read_avi_frames(video)
    assert len(back) == 2
    for i, data in enumerate(back):
        png = np.asarray(Image.open(os.path.join(out, "cameras", "%06d.png" % i)))
        assert data == je.encode(png, 80, "4:2:0", 1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "visualize.py"), "--synthetic", "--small", "--frames", "1", "--device",
                        "cpu", "--out", out + "2", "--video", video, "--video-stream", "bev", "--no-png"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(out + "2") or not os.listdir(out + "2")
    assert je.jpeg_size(je.read_avi_frames(video)[0]) == (1000, 1000)
