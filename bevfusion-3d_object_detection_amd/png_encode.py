"""Lossless PNG encode of 8-bit RGB frames (csrc/png_encode_host.h, csrc/png_encode.hip) in a restricted DEFLATE that runs in parallel.

This module DEFINES the format, in integer numpy; the C++ host path and the kernels reproduce it byte for byte.

`torch_png_filter(rgb)`: per row the filter type -- None, Sub, Up, Average, Paeth, all over the RAW row above; the row above the
first and the bytes left of the first pixel are zero -- with the least sum of `v < 128 ? v : 256 - v` over its filtered bytes
(libpng's heuristic), the lowest type on a tie; uint8 [H, 1 + 3 W], the type in front of each row.  Rows are independent.

`deflate_rle(data, band_bytes)`: a zlib stream (78 01 ... Adler-32) of one DEFLATE block per band of `band_bytes` bytes, every
band on a byte boundary, so that bands are coded -- and can be inflated -- independently:
  tokens   `run_tokens`: inside a band a maximal stretch of equal bytes is a literal, then matches of distance 1 and length
           min(r, 258) while r >= 3 bytes remain, then 0-2 literals.  No other matches.
  codes    `huffman_lengths`: a 15-bit length-limited prefix code over the band's 286-symbol histogram (end-of-block counts
           once) by package-merge, ties by symbol index; canonical codes (RFC 1951 3.2.2).  The distance alphabet is one code of
           one bit when the band has a match, and no code otherwise.
  dynamic  BFINAL (last band), BTYPE 10, HLIT 29, HDIST 0, HCLEN 15, a code-length code that gives symbols 0-15 four bits and
           16-18 none (complete; the code of length L is L), the 286 + 1 lengths on four bits each: HEADER_BITS = 1222; the
           tokens; end-of-block; and, unless it is the last band, an empty stored block: 000, pad, 00 00 FF FF.
  stored   a band whose dynamic form is not smaller than stored_bytes(n) = n + 5 ceil(n / 65535) goes out as stored blocks.
So no band takes more than stored_bytes(n), and `default_capacity` -- 2 + the sum of that over the bands -- is never exceeded:
there is no overflow-and-retry path.  The Adler-32 is combined on the host from one (A, B, n) triple per band.

`encode(rgb, band_rows)` is the whole file on the host: signature, IHDR (8-bit, colour type 2, no interlace), ONE IDAT, IEND,
the CRCs by zlib.crc32; a band is `band_rows` whole filtered rows (default: the fewest that give 64 KiB).  native=True runs the
same two stages in plain C++ (bfhip_png_filter_host, bfhip_png_deflate_host).

`fused_png_encode` is the device path: ONE upload (the descriptor table), bfhip_png_encode's four launches for the whole batch
-- frames of any sizes together -- and ONE host read (lengths, flags, Adler triples); then exactly that many bytes are copied.
`encode_frames` dispatches (BFHIP_PNG_ENCODE, ships on) and gives the same bytes either way.
"""
import ctypes
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib

ENABLED = os.environ.get("BFHIP_PNG_ENCODE", "1") != "0"
PATHS = {"kernel": 0, "torch": 0}  # batches by path

SYMBOLS, EOB, MAX_LEN, MAX_MATCH = 286, 256, 15, 258
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 4 * SYMBOLS + 4
ADLER_MOD = 65521
MIN_BAND_BYTES = 65536
MAX_BAND_BYTES = 1 << 26
FLAG_OVERFLOW = 1
RESULT_WORDS, BAND_WORDS = 8, 4
SIGNATURE = b"\x89PNG\r\n\x1a\n"


class Stats(ctypes.Structure):
    """bfhip_png_stats (include/bevfusion_hip.h)."""
    _fields_ = [("bytes", ctypes.c_int64), ("bands", ctypes.c_int64), ("stored_bands", ctypes.c_int64),
                ("dynamic_bands", ctypes.c_int64), ("tokens", ctypes.c_int64), ("max_code_length", ctypes.c_int32),
                ("overflow", ctypes.c_int32)]


class _Frame(ctypes.Structure):
    """bfhip_png_frame (include/bevfusion_hip.h)."""
    _fields_ = [("src_off", ctypes.c_int64), ("out_off", ctypes.c_int64), ("capacity", ctypes.c_int64), ("ws_off", ctypes.c_int64),
                ("res_off", ctypes.c_int64), ("n_bytes", ctypes.c_int64), ("band_bytes", ctypes.c_int64), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32)]


# ---------------------------------------------------------------------------------------------- sizes
def stored_bytes(n):
    """A band of n bytes as stored blocks of at most 65535 bytes, five bytes of header each."""
    return n + 5 * ((n + 65534) // 65535)


def default_band_rows(width, height):
    """The fewest whole rows that give at least 64 KiB of filtered bytes, at most the frame."""
    row = 1 + 3 * int(width)
    return max(1, min(int(height), -(-MIN_BAND_BYTES // row)))


def _band_rows(width, height, band_rows):
    if band_rows is None:
        return default_band_rows(width, height)
    if int(band_rows) < 1:
        raise ValueError("png encode: band_rows=%r" % (band_rows,))
    return min(int(band_rows), int(height))


def stream_capacity(n, band_bytes):
    """The most bytes 78 01 and the bands of n bytes can take: every band is at most its stored form, whichever form it has."""
    full, rest = divmod(int(n), int(band_bytes))
    return 2 + full * stored_bytes(int(band_bytes)) + (stored_bytes(rest) if rest else 0)


def default_capacity(width, height, band_rows=None):
    """Bytes set aside on the device for a frame's stream (without the Adler-32, which the host appends): with n_b the bytes of
    band b, 2 + sum_b (n_b + 5 ceil(n_b / 65535)).  A dynamic band is chosen only when it is smaller than its stored form, so
    this is a bound, not an estimate."""
    row = 1 + 3 * int(width)
    return stream_capacity(row * int(height), row * _band_rows(width, height, band_rows))


# ---------------------------------------------------------------------------------------------- the filter
def _as_rgb(rgb, who):
    if torch.is_tensor(rgb):
        if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
            raise ValueError("%s: uint8 [H, W, 3] with H, W >= 1 expected, got %s %s" % (who, tuple(rgb.shape), rgb.dtype))
        return rgb.cpu().contiguous().numpy()
    arr = np.asarray(rgb)
    if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3 or arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError("%s: uint8 [H, W, 3] with H, W >= 1 expected, got %s %s" % (who, tuple(arr.shape), arr.dtype))
    return np.ascontiguousarray(arr)


def torch_png_filter(rgb, chunk_rows=64):
    """uint8 [H, W, 3] (numpy or torch) -> uint8 [H, 1 + 3 W]: the chosen filter type and the filtered bytes of every row."""
    rgb = _as_rgb(rgb, "torch_png_filter")
    H, W = rgb.shape[:2]
    raw = rgb.reshape(H, 3 * W)
    out = np.empty((H, 1 + 3 * W), np.uint8)
    for y0 in range(0, H, chunk_rows):
        x = raw[y0:y0 + chunk_rows].astype(np.int32)
        a = np.zeros_like(x)
        a[:, 3:] = x[:, :-3]
        b = np.zeros_like(x)
        if y0:
            b[0] = raw[y0 - 1]
        b[1:] = x[:-1]
        c = np.zeros_like(x)
        c[:, 3:] = b[:, :-3]
        pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        cands = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255  # [5, rows, 3 W]
        cost = np.where(cands < 128, cands, 256 - cands).sum(2, dtype=np.int64)
        types = np.argmin(cost, 0)  # the first minimum: the lowest type on a tie
        out[y0:y0 + chunk_rows, 0] = types
        out[y0:y0 + chunk_rows, 1:] = np.take_along_axis(cands, types[None, :, None], 0)[0]
    return out


# ---------------------------------------------------------------------------------------------- tokens and codes
def run_tokens(band):
    """Bytes of ONE band -> (lit, length), one entry a token: a literal has its byte in `lit` and length 0; a match (always of
    distance 1) has lit -1 and its length 3 .. 258."""
    d = np.frombuffer(bytes(band), np.uint8) if not isinstance(band, np.ndarray) else band.reshape(-1)
    n = d.size
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    starts = np.concatenate([[0], np.flatnonzero(d[1:] != d[:-1]) + 1])
    runs = np.diff(np.concatenate([starts, [n]]))
    r = runs - 1
    q, rem = r // MAX_MATCH, r % MAX_MATCH
    count = 1 + q + np.where(rem >= 3, 1, rem)
    first = np.cumsum(count) - count
    run_of = np.repeat(np.arange(starts.size), count)
    j = np.arange(int(count.sum())) - first[run_of]  # the token's place in its stretch
    qj, remj = q[run_of], rem[run_of]
    length = np.where(j == 0, 0, np.where(j <= qj, MAX_MATCH, np.where(remj >= 3, remj, 0)))
    lit = np.where(length == 0, d[starts][run_of].astype(np.int32), -1)
    return lit.astype(np.int32), length.astype(np.int32)


def length_symbol(length):
    """Match lengths 3 .. 258 (array) -> (symbol 257 .. 285, number of extra bits, their value), RFC 1951 3.2.5."""
    length = np.asarray(length, np.int64)
    v = length - 3
    top = np.zeros_like(v)
    for k in range(1, 8):
        top = np.where(v >> k > 0, k, top)  # floor(log2 v)
    e = np.where(v < 8, 0, top - 2)
    sym = np.where(v < 8, 257 + v, 257 + 4 * (e + 1) + ((v >> e) & 3))
    extra = np.where(v < 8, 0, v & ((1 << e) - 1))
    last = length == MAX_MATCH
    return np.where(last, 285, sym), np.where(last, 0, e), np.where(last, 0, extra)


def _extra_bits_of(sym):
    return 0 if sym < 265 or sym == 285 else (sym - 261) >> 2


def huffman_lengths(hist, max_len=MAX_LEN):
    """Code lengths of a prefix code for the symbols with hist > 0, none longer than max_len and the cost sum(hist * length) the
    least possible under that limit: package-merge.  0 for an unused symbol; a single used symbol gets one bit; with two or more
    the code is complete (Kraft sum 1).  A deterministic function of the histogram:
      the used symbols in ascending order of (count, symbol) are the leaves; list 0 is the leaves; list l is the leaves merged
      with the pairs (items 2k, 2k + 1) of list l - 1, a leaf before a package of the same weight, cut at 2 n - 2 items; the first
      2 n - 2 items of list max_len - 1 are selected, and every selected package selects its two items one list down; a symbol's
      length is the number of lists in which its leaf is selected."""
    hist = [int(h) for h in hist]
    order = sorted((h, s) for s, h in enumerate(hist) if h > 0)
    n = len(order)
    lens = [0] * len(hist)
    if n == 0:
        return lens
    if n == 1:
        lens[order[0][1]] = 1
        return lens
    if (1 << max_len) < n:
        raise ValueError("huffman_lengths: %d symbols do not fit codes of %d bits" % (n, max_len))
    w = [h for h, _ in order]
    keep = 2 * n - 2
    lists, prev = [], []
    for _ in range(max_len):
        packages = [prev[2 * k] + prev[2 * k + 1] for k in range(len(prev) // 2)]
        cur, leaf, i, k = [], [], 0, 0
        while len(cur) < keep and (i < n or k < len(packages)):
            if i < n and (k >= len(packages) or w[i] <= packages[k]):
                cur.append(w[i])
                leaf.append(True)
                i += 1
            else:
                cur.append(packages[k])
                leaf.append(False)
                k += 1
        lists.append(leaf)
        prev = cur
    take = keep
    for leaf in reversed(lists):
        leaves = sum(leaf[:take])
        for r in range(leaves):
            lens[order[r][1]] += 1
        take = 2 * (take - leaves)
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2: code of every symbol with a length, as an integer whose most significant bit goes out first."""
    count = [0] * (MAX_LEN + 2)
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * (MAX_LEN + 2), 0
    for b in range(1, MAX_LEN + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            codes[s] = nxt[v]
            nxt[v] += 1
    return codes


def _reverse(v, n):
    return int(format(v, "0%db" % n)[::-1], 2) if n else 0


def _pack(values, lengths):
    """Pieces (value, number of bits), LSB first, into bytes; the last byte is padded with zero bits."""
    values, lengths = np.asarray(values, np.int64), np.asarray(lengths, np.int64)
    keep = lengths > 0
    values, lengths = values[keep], lengths[keep]
    start = np.cumsum(lengths) - lengths
    within = np.arange(int(lengths.sum())) - np.repeat(start, lengths)
    bits = (np.repeat(values, lengths) >> within) & 1
    return np.packbits(bits.astype(np.uint8), bitorder="little").tobytes(), int(lengths.sum())


def _band(d, final):
    """One band -> (its bytes in the stream, stored?)."""
    n = d.size
    lit, length = run_tokens(d)
    is_match = length > 0
    sym = lit.copy()
    msym, mne, mex = length_symbol(length[is_match])
    sym[is_match] = msym
    hist = np.bincount(sym, minlength=SYMBOLS)
    hist[EOB] = 1
    lens = huffman_lengths(hist)
    has_match = bool(is_match.any())
    bits = HEADER_BITS + int(is_match.sum()) + sum(int(hist[s]) * (lens[s] + (_extra_bits_of(s) if s > EOB else 0)) for s in range(SYMBOLS))
    dyn_bytes = (bits + 7) // 8 if final else (bits + 3 + 7) // 8 + 4
    if dyn_bytes >= stored_bytes(n):
        out = []
        raw = d.tobytes()
        for at in range(0, n, 65535):
            part = raw[at:at + 65535]
            out.append(struct.pack("<BHH", 1 if final and at + len(part) == n else 0, len(part), len(part) ^ 0xFFFF) + part)
        return b"".join(out), True
    codes = canonical_codes(lens)
    rev = np.array([_reverse(c, v) for c, v in zip(codes, lens)], np.int64)
    lens_a = np.array(lens, np.int64)
    head_v = [1 if final else 0, 2, 29, 0, 15] + [4 if s < 16 else 0 for s in CL_ORDER] + [_reverse(v, 4) for v in lens] + \
        [_reverse(1 if has_match else 0, 4)]
    head_l = [1, 2, 5, 5, 4] + [3] * 19 + [4] * (SYMBOLS + 1)
    T = sym.size
    vals = np.zeros((T + 1, 3), np.int64)
    nbits = np.zeros((T + 1, 3), np.int64)
    vals[:T, 0], nbits[:T, 0] = rev[sym], lens_a[sym]
    vals[:T, 1][is_match], nbits[:T, 1][is_match] = mex, mne
    nbits[:T, 2] = is_match  # the distance code: one 0 bit
    vals[T, 0], nbits[T, 0] = rev[EOB], lens_a[EOB]
    body, total = _pack(np.concatenate([head_v, vals.reshape(-1)]), np.concatenate([head_l, nbits.reshape(-1)]))
    assert total == bits
    if not final:
        body = body[:(bits + 3 + 7) // 8].ljust((bits + 3 + 7) // 8, b"\0") + b"\x00\x00\xff\xff"
    assert len(body) == dyn_bytes
    return body, False


def adler32_combine(a1, b1, a2, b2, n2):
    """(A, B) of a string followed by n2 more bytes whose own sums, started from (1, 0), are (a2, b2)."""
    return (a1 + a2 - 1) % ADLER_MOD, (b1 + b2 + n2 * (a1 - 1)) % ADLER_MOD


def adler32_of_bands(bands):
    """bands: (A, B, n, ...) per band -> the stream's Adler-32."""
    a, b = 1, 0
    for band in bands:
        a, b = adler32_combine(a, b, int(band[0]), int(band[1]), int(band[2]))
    return (b << 16) | a


def _check_deflate_args(n, band_bytes):
    if n < 1 or n >= 1 << 31 or not 1 <= int(band_bytes) <= MAX_BAND_BYTES:
        raise ValueError("deflate_rle: %d bytes in bands of %d: 1 .. 2^31 - 1 bytes in bands of 1 .. 2^26" % (n, band_bytes))


def _offsets(bands):
    offsets = [2]
    for band in bands:
        offsets.append(offsets[-1] + int(band[3]))
    return offsets


def deflate_bands(data, band_bytes):
    """The specification: data -> (78 01 and the bands, [(A, B, n, bytes, stored)] per band)."""
    d = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1)
    _check_deflate_args(d.size, band_bytes)
    band_bytes = int(band_bytes)
    out, bands = [b"\x78\x01"], []
    for at in range(0, d.size, band_bytes):
        part = d[at:at + band_bytes]
        body, stored = _band(part, at + band_bytes >= d.size)
        ad = zlib.adler32(part.tobytes())
        bands.append((ad & 0xFFFF, ad >> 16, part.size, len(body), stored))
        out.append(body)
    return b"".join(out), bands


def deflate_rle(data, band_bytes):
    """Any byte string -> (zlib stream, band offsets): offsets[b] is where band b begins in the stream, offsets[-1] where the
    Adler-32 trailer begins."""
    body, bands = deflate_bands(data, band_bytes)
    return body + struct.pack(">I", adler32_of_bands(bands)), _offsets(bands)


def host_deflate(data, band_bytes, capacity=None):
    """deflate_rle in plain C++ (bfhip_png_deflate_host): (zlib stream, band offsets, bands [(A, B, n, bytes, stored)], Stats)."""
    d = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1))
    _check_deflate_args(d.size, band_bytes)
    n_bands = -(-d.size // int(band_bytes))
    cap = stream_capacity(d.size, band_bytes) if capacity is None else int(capacity)
    out = np.empty(max(cap, 1), np.uint8)
    words = np.zeros((n_bands, BAND_WORDS), np.uint32)
    stats = Stats()
    _lib.call("bfhip_png_deflate_host", d.ctypes.data, d.size, int(band_bytes), out.ctypes.data, cap, words.ctypes.data, n_bands,
              ctypes.addressof(stats))
    bands = _bands_of(words)
    return out[:stats.bytes].tobytes() + struct.pack(">I", adler32_of_bands(bands)), _offsets(bands), bands, stats


def _bands_of(words):
    return [(int(w[0]), int(w[1]), int(w[2]), int(w[3]) & 0x7FFFFFFF, bool(int(w[3]) >> 31)) for w in words]


def host_filter(rgb):
    """torch_png_filter in plain C++ (bfhip_png_filter_host)."""
    rgb = _as_rgb(rgb, "host_filter")
    H, W = rgb.shape[:2]
    out = np.empty((H, 1 + 3 * W), np.uint8)
    _lib.call("bfhip_png_filter_host", rgb.ctypes.data, W, H, out.ctypes.data, out.size)
    return out


# ---------------------------------------------------------------------------------------------- the file
def _chunk(tag, payload):
    return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload) & 0xFFFFFFFF)


def png_file(width, height, stream):
    """Signature, IHDR (8-bit RGB, no interlace), one IDAT with the zlib stream, IEND."""
    return SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", int(width), int(height), 8, 2, 0, 0, 0)) + _chunk(b"IDAT", bytes(stream)) + \
        _chunk(b"IEND", b"")


def encode(rgb, band_rows=None, native=True):
    """uint8 [H, W, 3] -> the bytes of a PNG file, on the host: the specification (native=False) or the same in plain C++."""
    rgb = _as_rgb(rgb, "png encode")
    H, W = rgb.shape[:2]
    band_bytes = (1 + 3 * W) * _band_rows(W, H, band_rows)
    if native:
        stream = host_deflate(host_filter(rgb), band_bytes)[0]
    else:
        stream = deflate_rle(torch_png_filter(rgb), band_bytes)[0]
    return png_file(W, H, stream)


# ---------------------------------------------------------------------------------------------- the device path
class EncodeBatch:
    """The descriptor table of a batch and the buffers it addresses.  jobs: (width, height, band_rows or None) per frame, or --
    deflate=True -- (n_bytes, band_bytes) per byte string.  A stream gets the proved capacity unless `capacities` names one;
    `guard` bytes follow every stream; fill: a byte value the workspace and the output are filled with first."""

    def __init__(self, jobs, device, deflate=False, capacities=None, guard=0, fill=None):
        self.device = torch.device(device)
        self.deflate = deflate
        self.n = n = len(jobs)
        lib = _lib.load()
        if not 1 <= n <= lib.bfhip_png_encode_max_frames():
            raise ValueError("png encode: %d frames in one batch, 1 .. %d expected" % (n, lib.bfhip_png_encode_max_frames()))
        self.staging = torch.zeros(ctypes.sizeof(_Frame) * n, dtype=torch.uint8).pin_memory()
        self.descs = (_Frame * n).from_buffer(self.staging.numpy())
        src_at = out_at = ws_at = res_at = 0
        for i, (d, job) in enumerate(zip(self.descs, jobs)):
            if deflate:
                n_bytes, band_bytes = int(job[0]), int(job[1])
                _check_deflate_args(n_bytes, band_bytes)
                src = n_bytes
            else:
                w, h = int(job[0]), int(job[1])
                rows = _band_rows(w, h, job[2])
                if not lib.bfhip_png_encode_supported(w, h, rows):
                    raise ValueError("png encode: frame %d: %dx%d in bands of %d rows is not supported" % (i, w, h, rows))
                d.width, d.height = w, h
                n_bytes, band_bytes, src = (1 + 3 * w) * h, (1 + 3 * w) * rows, 3 * w * h
            d.n_bytes, d.band_bytes = n_bytes, band_bytes
            d.src_off, d.out_off, d.ws_off, d.res_off = src_at, out_at, ws_at, res_at
            d.capacity = stream_capacity(n_bytes, band_bytes) if capacities is None or capacities[i] is None else int(capacities[i])
            src_at += src
            out_at += (d.capacity + 15) // 16 * 16 + guard
            ws_at += _lib.call_size("bfhip_png_workspace_bytes", n_bytes, band_bytes, 0 if deflate else 1)
            res_at += _lib.call_size("bfhip_png_result_words", n_bytes, band_bytes)
        self.src_bytes, self.out_bytes, self.ws_bytes, self.res_words, self.guard = src_at, max(out_at, 16), ws_at, res_at, guard
        self.table = self.staging.to(self.device, non_blocking=True)  # the batch's one upload
        make = (lambda m, dt: torch.full((m,), fill, dtype=dt, device=self.device)) if fill is not None else \
            (lambda m, dt: torch.empty(m, dtype=dt, device=self.device))
        self.workspace = make(self.ws_bytes, torch.uint8)
        self.out = make(self.out_bytes, torch.uint8)
        self.result = torch.zeros(self.res_words, dtype=torch.int32, device=self.device)

    def run(self, src):
        """src: the frames' pixels, or the byte strings, end to end in one uint8 tensor on the device."""
        with torch.cuda.device(self.device):
            _lib.call("bfhip_png_deflate" if self.deflate else "bfhip_png_encode", ctypes.addressof(self.descs), self.table.data_ptr(),
                      self.n, src.data_ptr(), src.numel(), self.workspace.data_ptr(), self.workspace.numel(), self.out.data_ptr(),
                      self.out.numel(), self.result.data_ptr(), self.result.numel(), _lib.stream_of(self.out))

    def streams(self):
        """The one host read, then each job's bytes: [(zlib stream with its Adler-32 or None on overflow, length without the
        trailer, flags, bands [(A, B, n, bytes, stored)], header words)]."""
        res = self.result.cpu().numpy().view(np.uint32)
        got = []
        for d in self.descs:
            head = [int(v) for v in res[d.res_off:d.res_off + RESULT_WORDS]]
            length, flags = head[0] | (head[1] << 32), head[2]
            bands = _bands_of(res[d.res_off + RESULT_WORDS:d.res_off + RESULT_WORDS + BAND_WORDS * head[6]].reshape(-1, BAND_WORDS))
            data = None
            if not flags & FLAG_OVERFLOW:
                data = self.out[d.out_off:d.out_off + length].cpu().numpy().tobytes() + struct.pack(">I", adler32_of_bands(bands))
            got.append((data, length, flags, bands, head))
        return got


def _flat(tensors, device):
    tensors = [t.contiguous().view(-1) for t in tensors]
    for t in tensors:
        if t.dtype != torch.uint8 or t.device != device:
            raise ValueError("png encode: uint8 tensors on %s expected, got %s on %s" % (device, t.dtype, t.device))
    return tensors[0] if len(tensors) == 1 else torch.cat(tensors)


def fused_png_encode(frames, band_rows=None, capacity=None, guard=0, fill=None, _batch_out=None):
    """frames: list of uint8 [H, W, 3] tensors on one GPU -> list of bytes (whole PNG files).  band_rows / capacity: one value or
    a list with one per frame.  A frame whose stream outgrew a capacity the caller named comes back as (None, needed length)."""
    n = len(frames)
    rows = band_rows if isinstance(band_rows, list) else [band_rows] * n
    capacities = capacity if isinstance(capacity, list) else [capacity] * n
    for f in frames:
        _check_frame(f)
    device = frames[0].device
    batch = EncodeBatch([(f.shape[1], f.shape[0], r) for f, r in zip(frames, rows)], device, False, capacities, guard, fill)
    batch.run(_flat(frames, device))
    if _batch_out is not None:
        _batch_out.append(batch)
    return [(None, length) if data is None else png_file(f.shape[1], f.shape[0], data)
            for f, (data, length, _, _, _) in zip(frames, batch.streams())]


def fused_deflate(strings, band_bytes, capacity=None, guard=0, fill=None, _batch_out=None):
    """strings: list of 1-D uint8 tensors on one GPU -> [(zlib stream, band offsets, bands)] (bfhip_png_deflate); a stream that
    outgrew a capacity the caller named comes back as (None, needed length, bands)."""
    n = len(strings)
    sizes = band_bytes if isinstance(band_bytes, list) else [band_bytes] * n
    capacities = capacity if isinstance(capacity, list) else [capacity] * n
    device = strings[0].device
    batch = EncodeBatch([(s.numel(), b) for s, b in zip(strings, sizes)], device, True, capacities, guard, fill)
    batch.run(_flat(strings, device))
    if _batch_out is not None:
        _batch_out.append(batch)
    return [(data, length if data is None else _offsets(bands), bands) for data, length, _, bands, _ in batch.streams()]


def _check_frame(f):
    if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
        shape, dtype = (tuple(f.shape), f.dtype) if hasattr(f, "shape") else (None, type(f))
        raise ValueError("png encode: uint8 [H, W, 3] tensors with H, W >= 1 expected, got %s %s" % (shape, dtype))


def encode_frames(frames, band_rows=None):
    """list of uint8 [H, W, 3] tensors -> list of bytes (PNG files): the kernels for device tensors (BFHIP_PNG_ENCODE, ships on),
    `encode` on the host otherwise; the same bytes either way."""
    frames = list(frames)
    most = _lib.load().bfhip_png_encode_max_frames()
    if len(frames) > most:
        raise ValueError("png encode: %d frames in one batch, at most %d" % (len(frames), most))
    for f in frames:
        _check_frame(f)
    if not frames:
        return []
    if ENABLED and all(f.is_cuda for f in frames):
        PATHS["kernel"] += 1
        return fused_png_encode(frames, band_rows)
    PATHS["torch"] += 1
    return [encode(f, band_rows) for f in frames]


def write_frames(paths, frames, band_rows=None):
    """Encodes the frames together and writes one file each."""
    paths, frames = list(paths), list(frames)
    if len(paths) != len(frames):
        raise ValueError("write_frames: %d paths for %d frames" % (len(paths), len(frames)))
    for path, data in zip(paths, encode_frames(frames, band_rows)):
        with open(path, "wb") as f:
            f.write(data)
