"""Shared by tests/test_png_encode_cpu.py and tests/test_png_encode_gpu.py: the frames, the byte strings, and independent readers
of what the encoder writes (a chunk walker, a token reader for the restricted DEFLATE, a loop-written filter heuristic)."""
import os
import struct
import zlib

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "nus_cam_front.jpg")
BAND_ROWS = (1, 2, 7, None)
STRETCHES = (1, 2, 3, 4, 258, 259, 260, 261, 517)
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def frames():
    """name -> uint8 [H, W, 3]: the smallest frames at which each mechanism of the encoder can go wrong (width x height)."""
    rs = np.random.RandomState(7)
    out = {}
    for w, h in ((1, 1), (1, 7), (7, 1), (2, 3)):  # left neighbours outside the row
        out["tiny_%dx%d" % (w, h)] = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    out["flat_87x2"] = np.full((2, 87, 3), 93, np.uint8)    # match splitting and the 1-2 byte tail
    out["flat_300x5"] = np.full((5, 300, 3), 200, np.uint8)  # runs across rows, Up against None
    out["noise_64x64"] = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)  # the stored band
    half = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    half[:, 32:] = 17
    out["half_64x64"] = half                                 # a dynamic band with 256 literals in use
    x = np.arange(33, dtype=np.int64)
    out["hramp_33x9"] = np.broadcast_to(((x * 7) % 256)[None, :, None], (9, 33, 3)).astype(np.uint8).copy()  # Sub
    y = np.arange(9, dtype=np.int64)
    base = ((np.arange(33)[:, None] * 37 + np.arange(3)[None, :] * 5) % 100)[None]  # neighbours differ by 37 or 63; climbs 11 a row:
    out["vramp_33x9"] = (base + 11 * y[:, None, None]).astype(np.uint8)  # Up leaves 11s, and so does Paeth: the tie goes to Up
    yy, xx = np.mgrid[0:40, 0:40]
    smooth = (3 * xx + 2 * yy)[..., None] + np.array([0, 40, 90]) + rs.randint(-2, 3, (40, 40, 3))
    out["smooth_40x40"] = np.clip(smooth, 0, 255).astype(np.uint8)  # Paeth or Average
    return out


def fixture_frame():
    from PIL import Image
    return np.asarray(Image.open(FIXTURE).convert("RGB"), np.uint8).copy()


def _spread(counts):
    """Bytes in which value s occurs counts[s] times and no two neighbours are equal: the most frequent value first, on every other
    position."""
    total = sum(counts)
    assert max(counts) <= (total + 1) // 2
    out = np.zeros(total, np.uint8)
    spots = list(range(0, total, 2)) + list(range(1, total, 2))
    at = 0
    for s in sorted(range(len(counts)), key=lambda s: -counts[s]):
        out[spots[at:at + counts[s]]] = s
        at += counts[s]
    assert (out[1:] != out[:-1]).all()
    return out.tobytes()


def fibonacci_string(symbols=20):
    """Values 0 .. symbols - 1 occur 1, 1, 2, 3, 5 ... times, all as literals."""
    fib = [1, 1]
    while len(fib) < symbols:
        fib.append(fib[-1] + fib[-2])
    return _spread(fib)


def doubling_string(symbols=18):
    """Value s occurs 2^s times, all as literals: with end-of-block the only optimal unlimited code is a chain `symbols` deep, so
    for 18 symbols the 15-bit limit binds (a Fibonacci histogram with one more count of 1 has shallow optimal codes too)."""
    return _spread([1 << s for s in range(symbols)])


def stretch_string(length):
    return b"\x07" + b"A" * length + b"\x09"


def expected_tokens(band):
    """The rule, written as a loop: ('lit', byte) and ('match', length) for one band."""
    out, i, n = [], 0, len(band)
    while i < n:
        e = i
        while e < n and band[e] == band[i]:
            e += 1
        out.append(("lit", band[i]))
        r = e - i - 1
        while r >= 3:
            out.append(("match", min(r, 258)))
            r -= min(r, 258)
        out.extend([("lit", band[i])] * r)
        i = e
    return out


class _Bits:
    def __init__(self, data, at=0):
        self.data, self.at = data, at * 8

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.data[(self.at + k) >> 3] >> ((self.at + k) & 7)) & 1) << k
        self.at += n
        return v


def read_band(stream, begin):
    """One band of the restricted DEFLATE from byte `begin` of the zlib stream: ('stored', bytes, final, end) or ('dynamic',
    tokens, final, end, lens) -- read with nothing but RFC 1951."""
    bits = _Bits(stream, begin)
    final, btype = bits.take(1), bits.take(2)
    if btype == 0:
        data = b""
        at = begin
        while True:
            fin, n, nn = stream[at], struct.unpack_from("<H", stream, at + 1)[0], struct.unpack_from("<H", stream, at + 3)[0]
            assert fin in (0, 1) and n ^ nn == 0xFFFF
            data += stream[at + 5:at + 5 + n]
            at += 5 + n
            if n < 65535 or fin:
                return ("stored", data, fin, at)
    assert btype == 2
    assert (bits.take(5), bits.take(5), bits.take(4)) == (29, 0, 15)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    assert [bits.take(3) for _ in order] == [0 if s > 15 else 4 for s in order]
    rev4 = lambda v: int(format(v, "04b")[::-1], 2)  # noqa: E731
    lens = [rev4(bits.take(4)) for _ in range(286)]
    dist = rev4(bits.take(4))
    assert dist in (0, 1)
    count = [0] * 17
    for v in lens:
        count[v] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, v in enumerate(lens):
        if v:
            table[(v, nxt[v])] = s
            nxt[v] += 1
    tokens = []
    while True:
        code, n = 0, 0
        while (n, code) not in table:
            code, n = (code << 1) | bits.take(1), n + 1
            assert n <= 15
        s = table[(n, code)]
        if s < 256:
            tokens.append(("lit", s))
        elif s == 256:
            break
        else:
            tokens.append(("match", LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])))
            assert dist == 1 and bits.take(1) == 0
    end = (bits.at + 7) // 8
    if not final:
        assert bits.take(3) == 0
        end = (bits.at + 7) // 8
        assert stream[end:end + 4] == b"\x00\x00\xff\xff"
        end += 4
    return ("dynamic", tokens, final, end, lens)


def chunks(png):
    """[(tag, payload)] of a PNG file; every length and CRC is checked."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(png):
        n, tag = struct.unpack_from(">I4s", png, at)
        payload = png[at + 8:at + 8 + n]
        assert len(payload) == n
        assert struct.unpack_from(">I", png, at + 8 + n)[0] == zlib.crc32(tag + payload) & 0xFFFFFFFF
        out.append((tag, payload))
        at += 12 + n
    assert at == len(png)
    return out


def loop_filter_types(rgb):
    """The heuristic, written as loops over rows and bytes: the chosen type of every row."""
    H, W = rgb.shape[:2]
    raw = rgb.reshape(H, 3 * W).astype(int).tolist()
    types = []
    for y in range(H):
        cost = [0] * 5
        for i in range(3 * W):
            x = raw[y][i]
            a = raw[y][i - 3] if i >= 3 else 0
            b = raw[y - 1][i] if y else 0
            c = raw[y - 1][i - 3] if y and i >= 3 else 0
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            paeth = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            for t, p in enumerate((0, a, b, (a + b) // 2, paeth)):
                v = (x - p) % 256
                cost[t] += v if v < 128 else 256 - v
        types.append(cost.index(min(cost)))
    return types
