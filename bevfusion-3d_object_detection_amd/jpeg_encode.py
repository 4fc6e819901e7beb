"""Baseline JPEG encode and Motion-JPEG video (csrc/jpeg_encode_host.h, csrc/jpeg_encode.hip): jpeg.py turned round.

`torch_jpeg_forward(rgb, quant, hs, vs)` is the data-parallel half in numpy int32 and DEFINES the device stage
(bfhip_jpeg_forward): libjpeg's 16-bit fixed-point colour conversion (jccolor), its edge padding, its h2v2 / h2v1 chroma
downsampling with the alternating bias, its accurate integer forward DCT (jfdctint: CONST_BITS 13, PASS1_BITS 2; rows first,
columns second), its quantisation and the dummy blocks of its coefficient controller.  The coefficients come in the DECODER's
layout -- per component [block_rows, block_cols, 64] int16 at header.coef_offset[c], natural order, DC not differenced -- so
jpeg.torch_jpeg_decode(header, coef) decodes them and Pillow's coefficients (its file through jpeg.entropy_decode) compare
element for element: they are equal bit for bit (tests/test_jpeg_encode_cpu.py).

`build_stream(header, coef, restart_rows)` is the serial half: the host entropy encoder (bfhip_jpeg_entropy_encode: plain C++,
Annex K's Huffman tables) behind libjpeg's markers; with the coefficients above the file is byte for byte Pillow's
`save(quality=, subsampling=, restart_marker_rows=)`.  `encode` is both on the host.

`fused_jpeg_encode` is the device path: ONE upload (the descriptor table), bfhip_jpeg_encode's three launches for the whole
batch -- frames of any sizes, samplings and tables together -- and ONE host read (the lengths); then exactly that many bytes
are copied.  A restart marker follows every MCU row: the rows are what the Huffman stage runs in parallel.  `encode_frames`
dispatches (BFHIP_JPEG_ENCODE, ships on) and gives the same bytes either way.  `MjpegAviWriter` puts streams into an AVI file.
"""
import ctypes
import os
import struct

import numpy as np
import torch

from . import _lib
from . import jpeg

ENABLED = os.environ.get("BFHIP_JPEG_ENCODE", "1") != "0"
PATHS = {"kernel": 0, "torch": 0, "retried": 0}  # batches by path; frames encoded a second time after an overflow

SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
FLAG_OVERFLOW, FLAG_BAD_COEF = 1, 2

# Annex K: K.1 / K.2 in natural order
_BASE_QUANT = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99]], np.int64)
# zigzag position -> natural position
_NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# Annex K: K.3 - K.6, (codes per length 1..16, symbols in code order), in the order libjpeg writes them: DC0, AC0, DC1, AC1
_DHT = [
    (0x00, [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0x10, [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
     [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
      0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
      0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
      0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
    (0x01, [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (0x11, [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
     [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
      0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
      0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
      0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
      0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]),
]


class Stats(ctypes.Structure):
    """bfhip_jpeg_enc_stats (include/bevfusion_hip.h)."""
    _fields_ = [("bytes", ctypes.c_int64), ("stuffed", ctypes.c_int64), ("zrl", ctypes.c_int64), ("eob", ctypes.c_int64),
                ("max_ac_category", ctypes.c_int32), ("max_dc_category", ctypes.c_int32)]


class _EncFrame(ctypes.Structure):
    """bfhip_jpeg_enc_frame (include/bevfusion_hip.h)."""
    _fields_ = [("rgb_off", ctypes.c_int64), ("coef_off", ctypes.c_int64 * 3), ("out_off", ctypes.c_int64),
                ("capacity", ctypes.c_int64), ("ws_off", ctypes.c_int64), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("hs", ctypes.c_int32), ("vs", ctypes.c_int32), ("block_cols", ctypes.c_int32 * 3),
                ("block_rows", ctypes.c_int32 * 3), ("quant", (ctypes.c_uint16 * 64) * 3)]


def quant_tables(quality):
    """uint16 [2, 64], natural order: Annex K's luminance and chrominance tables under libjpeg's jpeg_quality_scaling."""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((_BASE_QUANT * s + 50) // 100, 1, 255).astype(np.uint16)


def _sampling(subsampling):
    if subsampling in SAMPLINGS:
        return SAMPLINGS[subsampling]
    if tuple(subsampling) in SAMPLINGS.values():
        return tuple(subsampling)
    raise ValueError("subsampling %r: one of %s" % (subsampling, ", ".join(SAMPLINGS)))


# ---------------------------------------------------------------------------------------------- the restatement
def _fdct_pass(v, first):
    """One pass of jfdctint's 8-point forward DCT along the last axis of an int32 array, wrap-around.  first: outputs 0 and 4
    shifted left by 2, the rest descaled by 11; otherwise 0 and 4 descaled by 2 and the rest by 15."""
    c = np.int32
    d = [v[..., k] for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    shift = 11 if first else 15
    half = c(1 << (shift - 1))
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << c(2), (t10 - t11) << c(2)
    else:
        out[0], out[4] = (t10 + t11 + c(2)) >> c(2), (t10 - t11 + c(2)) >> c(2)
    z1 = (t12 + t13) * c(4433)
    out[2] = (z1 + t13 * c(6270) + half) >> c(shift)
    out[6] = (z1 + t12 * c(-15137) + half) >> c(shift)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * c(9633)
    o4, o5, o6, o7 = t4 * c(2446), t5 * c(16819), t6 * c(25172), t7 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    out[7] = (o4 + z1 + z3 + half) >> c(shift)
    out[5] = (o5 + z2 + z4 + half) >> c(shift)
    out[3] = (o6 + z2 + z3 + half) >> c(shift)
    out[1] = (o7 + z1 + z4 + half) >> c(shift)
    return np.stack(out, -1)


def _blocks(plane, quant):
    """int32 plane [8 br, 8 bc] (samples 0..255) -> quantised int32 [br, bc, 64], natural order."""
    br, bc = plane.shape[0] // 8, plane.shape[1] // 8
    x = (plane - np.int32(128)).reshape(br, 8, bc, 8).transpose(0, 2, 1, 3)
    x = _fdct_pass(x, True)                                    # rows
    x = _fdct_pass(x.swapaxes(-1, -2), False).swapaxes(-1, -2)  # columns
    qv = (quant.astype(np.int32).reshape(8, 8) << np.int32(3))
    mag = (np.abs(x) + (qv >> np.int32(1))) // qv
    return np.where(x < 0, -mag, mag).reshape(br, bc, 64)


def _extend(plane, rows, cols):
    """Repeats the last row and column up to [rows, cols]."""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def torch_jpeg_forward(rgb, quant, hs, vs):
    """uint8 [H, W, 3] (numpy or torch), quant uint16 [2, 64] natural order (luma, chroma), luma sampling hs x vs ->
    (jpeg.Header, int16 coefficient vector) in the decoder's layout."""
    if torch.is_tensor(rgb):
        rgb = rgb.cpu().numpy()
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("torch_jpeg_forward: uint8 [H, W, 3] expected")
    hs, vs = _sampling((hs, vs))
    quant = np.asarray(quant)
    H, W = rgb.shape[:2]
    header = jpeg.make_header(W, H, hs, vs, [quant[0], quant[1], quant[1]])
    c = np.int32
    with np.errstate(over="ignore"):
        r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
        y = (c(19595) * r + c(38470) * g + c(7471) * b + c(32768)) >> c(16)
        cb = (c(-11059) * r + c(-21709) * g + c(32768) * b + c((128 << 16) + 32767)) >> c(16)
        cr = (c(32768) * r + c(-27439) * g + c(-5329) * b + c((128 << 16) + 32767)) >> c(16)
        planes = [_extend(y, header.block_rows[0] * 8, header.block_cols[0] * 8)]
        for p in (cb, cr):
            p = _extend(p, -(-H // vs) * vs, header.mcus_x * 8 * hs)  # whole MCUs to the right, a whole row group down
            if hs == 2 and vs == 2:
                bias = (c(1) + (np.arange(p.shape[1] // 2, dtype=np.int32) & c(1)))[None, :]
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> c(2)
            elif hs == 2:
                bias = (np.arange(p.shape[1] // 2, dtype=np.int32) & c(1))[None, :]
                p = (p[:, 0::2] + p[:, 1::2] + bias) >> c(1)
            planes.append(_extend(p, header.mcus_y * 8, header.mcus_x * 8))  # the DOWNSAMPLED plane's last row repeated
        coef = np.zeros(header.coef_bytes // 2, np.int16)
        for k, p in enumerate(planes):
            blocks = _blocks(p, quant[min(k, 1)])
            if k == 0 and (hs == 2 or vs == 2):  # libjpeg's dummy blocks: zero but for a DC copied from a neighbour
                real_rows, real_cols = -(-H // 8), -(-W // 8)
                for bx in range(real_cols, blocks.shape[1]):
                    blocks[:real_rows, bx, 1:] = 0
                    blocks[:real_rows, bx, 0] = blocks[:real_rows, bx - 1, 0]
                for by in range(real_rows, blocks.shape[0]):
                    blocks[by, :, 1:] = 0
                    for bx in range(blocks.shape[1]):
                        blocks[by, bx, 0] = blocks[by - 1, bx // hs * hs + hs - 1, 0]
            n = blocks.size
            coef[header.coef_offset[k]:header.coef_offset[k] + n] = blocks.reshape(-1).astype(np.int16)
    return header, coef


# ---------------------------------------------------------------------------------------------- the stream
def entropy_encode(header, coef, restart_interval=0, capacity=None):
    """bfhip_jpeg_entropy_encode: (bytes of the scan with its EOI, Stats).  restart_interval in MCUs.  RuntimeError when a
    coefficient has no Huffman code, the header is inconsistent or `capacity` is too small."""
    coef = np.ascontiguousarray(np.asarray(coef).reshape(-1))
    if coef.dtype != np.int16:
        raise TypeError("entropy_encode: int16 coefficients expected")
    stats = Stats()
    if capacity is None:  # the longest code of a block is 208 bytes, every one of which may be stuffed; markers, padding
        blocks = sum(header.block_cols[c] * header.block_rows[c] for c in range(3))
        capacity = blocks * 416 + 4 * header.mcus_x * header.mcus_y + 16
    out = np.empty(capacity, np.uint8)
    _lib.call("bfhip_jpeg_entropy_encode", ctypes.addressof(header), coef.ctypes.data, coef.nbytes, int(restart_interval),
              out.ctypes.data, out.size, ctypes.addressof(stats))
    return out[:stats.bytes].tobytes(), stats


def stream_headers(header, restart_interval=0):
    """The markers libjpeg writes in front of the scan: SOI, APP0 (JFIF 1.01, no density), one DQT per table, SOF0, the four
    DHT of Annex K, DRI when there are restarts, SOS."""
    q = header.quant_array()
    out = [b"\xff\xd8", b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)]
    for t, table in ((0, q[0]), (1, q[1])):
        out.append(b"\xff\xdb" + struct.pack(">HB", 67, t) + bytes(int(v) for v in table[_NATURAL]))
    out.append(b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, header.height, header.width, 3) +
               bytes([1, header.hs[0] << 4 | header.vs[0], 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in _DHT:
        out.append(b"\xff\xc4" + struct.pack(">HB", 19 + len(vals), tc_th) + bytes(bits) + bytes(vals))
    if restart_interval:
        out.append(b"\xff\xdd" + struct.pack(">HH", 4, restart_interval))
    out.append(b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return b"".join(out)


def _restart_interval(header, restart_rows):
    interval = int(restart_rows) * header.mcus_x
    if interval > 65535:
        raise ValueError("a restart interval of %d MCUs does not fit the DRI marker" % interval)
    return interval


def build_stream(header, coef, restart_rows=1):
    """The whole file: libjpeg's markers, the scan with a restart marker every `restart_rows` MCU rows (0: none), EOI."""
    interval = _restart_interval(header, restart_rows)
    if not np.array_equal(header.quant_array()[1], header.quant_array()[2]):
        raise ValueError("build_stream: the two chroma components share a quantisation table")
    return stream_headers(header, interval) + entropy_encode(header, coef, interval)[0]


def encode(rgb, quality=90, subsampling="4:2:0", restart_rows=1):
    """uint8 [H, W, 3] -> the bytes of a baseline JPEG file, on the host."""
    hs, vs = _sampling(subsampling)
    header, coef = torch_jpeg_forward(rgb, quant_tables(quality), hs, vs)
    return build_stream(header, coef, restart_rows)


# ---------------------------------------------------------------------------------------------- the device path
class EncodeBatch:
    """The descriptor table of a batch and the buffers it addresses; `frames` is a list of (width, height, hs, vs, quant [2 or 3,
    64]).  rgb_offs / capacities may be given; by default the pixels lie end to end and a stream gets `default_capacity`."""

    def __init__(self, frames, device, capacities=None, guard=0):
        self.device = torch.device(device)
        self.n = n = len(frames)
        if not 1 <= n <= _lib.load().bfhip_jpeg_encode_max_frames():
            raise ValueError("EncodeBatch: %d frames" % n)
        self.staging = torch.empty(ctypes.sizeof(_EncFrame) * n, dtype=torch.uint8).pin_memory()
        self.descs = (_EncFrame * n).from_buffer(self.staging.numpy())
        self.headers = []
        rgb_at = coef_at = out_at = ws_at = 0
        for i, (d, (w, h, hs, vs, quant)) in enumerate(zip(self.descs, frames)):
            if not _lib.load().bfhip_jpeg_encode_supported(int(w), int(h), int(hs), int(vs)):
                raise ValueError("EncodeBatch: frame %d: %dx%d sampling %dx%d is not supported" % (i, w, h, hs, vs))
            quant = np.asarray(quant)
            hd = jpeg.make_header(w, h, hs, vs, [quant[0], quant[1], quant[-1]])
            self.headers.append(hd)
            d.width, d.height, d.hs, d.vs = hd.width, hd.height, hs, vs
            d.rgb_off = rgb_at
            for c in range(3):
                d.coef_off[c] = coef_at + hd.coef_offset[c]
                d.block_cols[c], d.block_rows[c] = hd.block_cols[c], hd.block_rows[c]
            ctypes.memmove(d.quant, hd.quant, ctypes.sizeof(hd.quant))
            d.out_off = out_at
            d.capacity = default_capacity(w, h) if capacities is None or capacities[i] is None else int(capacities[i])
            d.ws_off = ws_at
            rgb_at += hd.width * hd.height * 3
            coef_at += hd.coef_bytes // 2
            out_at += (d.capacity + 15) // 16 * 16 + guard
            ws_at += _lib.call_size("bfhip_jpeg_encode_workspace_bytes", hd.width, hd.height, hs, vs)
        self.rgb_bytes, self.coef_elems, self.out_bytes, self.ws_bytes, self.guard = rgb_at, coef_at, out_at, ws_at, guard

    def upload(self):
        """The batch's one upload."""
        self.table = self.staging.to(self.device, non_blocking=True)
        return self.table

    def alloc(self, coef=True, entropy=True):
        dev = self.device
        if coef:
            self.coef = torch.empty(self.coef_elems, dtype=torch.int16, device=dev)
        if entropy:
            self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
            self.out = torch.full((self.out_bytes,), 0xA5, dtype=torch.uint8, device=dev) if self.guard else \
                torch.empty(self.out_bytes, dtype=torch.uint8, device=dev)
            self.result = torch.empty((self.n, 2), dtype=torch.int64, device=dev)

    def forward(self, rgb):
        with torch.cuda.device(self.device):
            _lib.call("bfhip_jpeg_forward", ctypes.addressof(self.descs), self.table.data_ptr(), self.n, rgb.data_ptr(), rgb.numel(),
                      self.coef.data_ptr(), self.coef.numel(), _lib.stream_of(self.coef))

    def entropy(self):
        with torch.cuda.device(self.device):
            _lib.call("bfhip_jpeg_entropy_encode_device", ctypes.addressof(self.descs), self.table.data_ptr(), self.n,
                      self.coef.data_ptr(), self.coef.numel(), self.workspace.data_ptr(), self.workspace.numel(), self.out.data_ptr(),
                      self.out.numel(), self.result.data_ptr(), _lib.stream_of(self.out))

    def encode(self, rgb):
        with torch.cuda.device(self.device):
            _lib.call("bfhip_jpeg_encode", ctypes.addressof(self.descs), self.table.data_ptr(), self.n, rgb.data_ptr(), rgb.numel(),
                      self.coef.data_ptr(), self.coef.numel(), self.workspace.data_ptr(), self.workspace.numel(), self.out.data_ptr(),
                      self.out.numel(), self.result.data_ptr(), _lib.stream_of(self.out))

    def frame_coef(self, i):
        d = self.descs[i]
        return self.coef[d.coef_off[0]:d.coef_off[0] + self.headers[i].coef_bytes // 2]

    def scans(self):
        """The one host read (the lengths and flags), then each frame's bytes: [(scan bytes or None on overflow, needed length,
        flags)]."""
        result = self.result.cpu().numpy()
        got = []
        for i, d in enumerate(self.descs):
            length, flags = int(result[i, 0]), int(result[i, 1])
            if flags & FLAG_BAD_COEF:
                raise RuntimeError("jpeg encode: frame %d holds a coefficient without a Huffman code" % i)
            data = None if flags & FLAG_OVERFLOW else self.out[d.out_off:d.out_off + length].cpu().numpy().tobytes()
            got.append((data, length, flags))
        return got


def default_capacity(width, height):
    """Bytes set aside for a frame's scan when the caller names none: as many as the pixels take (noise at quality 100 needs two
    thirds of that) and some; a stream that needs more reports its length and is encoded again."""
    return 3 * int(width) * int(height) + 4096


def _flat_pixels(frames, device):
    frames = [f.contiguous() for f in frames]
    for f in frames:
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.device != device:
            raise ValueError("jpeg encode: uint8 [H, W, 3] tensors on %s expected" % device)
    return frames[0].view(-1) if len(frames) == 1 else torch.cat([f.view(-1) for f in frames])


def fused_jpeg_encode(frames, quality=90, subsampling="4:2:0", capacity=None, guard=0, _batch_out=None):
    """frames: list of uint8 [H, W, 3] tensors on one GPU -> list of bytes (whole JPEG files, a restart marker every MCU row).
    quality / subsampling: one value, or a list with one per frame.  capacity: bytes set aside per scan (one value or a list;
    default_capacity otherwise); a frame whose scan needs more comes back as (None, needed length) instead of bytes."""
    n = len(frames)
    device = frames[0].device
    qualities = quality if isinstance(quality, list) else [quality] * n
    samplings = subsampling if isinstance(subsampling, list) else [subsampling] * n
    capacities = capacity if isinstance(capacity, list) else [capacity] * n
    specs = [(f.shape[1], f.shape[0]) + _sampling(s) + (quant_tables(q),) for f, q, s in zip(frames, qualities, samplings)]
    batch = EncodeBatch(specs, device, capacities, guard)
    batch.upload()
    batch.alloc()
    batch.encode(_flat_pixels(frames, device))
    if _batch_out is not None:
        _batch_out.append(batch)
    out = []
    for hd, (data, length, _) in zip(batch.headers, batch.scans()):
        out.append((None, length) if data is None else stream_headers(hd, hd.mcus_x) + data)
    return out


def encode_frames(frames, quality=90, subsampling="4:2:0", capacity=None):
    """list of uint8 [H, W, 3] tensors -> list of bytes: the device path on a GPU (BFHIP_JPEG_ENCODE, ships on), `encode` on the
    host otherwise; the same bytes either way.  A frame whose scan outgrew its capacity is encoded once more with the length it
    reported."""
    frames = list(frames)
    if ENABLED and frames and all(torch.is_tensor(f) and f.is_cuda for f in frames):
        PATHS["kernel"] += 1
        out = fused_jpeg_encode(frames, quality, subsampling, capacity)
        again = [i for i, o in enumerate(out) if isinstance(o, tuple)]
        if again:
            PATHS["retried"] += len(again)
            per = lambda v: [v[i] for i in again] if isinstance(v, list) else v  # noqa: E731
            redo = fused_jpeg_encode([frames[i] for i in again], per(quality), per(subsampling), [out[i][1] for i in again])
            for i, o in zip(again, redo):
                if isinstance(o, tuple):
                    raise RuntimeError("jpeg encode: frame %d needs %d bytes after it reported %d" % (i, o[1], out[i][1]))
                out[i] = o
        return out
    PATHS["torch"] += 1
    return [encode(f, quality, subsampling, 1) for f in frames]


# ---------------------------------------------------------------------------------------------- Motion-JPEG in AVI
AVI_LIMIT = (2 << 30) - (16 << 20)  # AVI 1.0: one RIFF chunk, 32-bit sizes; the index and the tail need room below 2 GB


class MjpegAviWriter:
    """An AVI 1.0 (RIFF) file with one Motion-JPEG video stream: hdrl (avih, one strl: strh vids/MJPG, strf BITMAPINFOHEADER
    with biCompression MJPG), movi (one word-aligned 00dc chunk a frame) and the idx1 index; the sizes and the frame count are
    patched in by close().  write() takes the bytes of one JPEG file of the constructor's size."""

    def __init__(self, path, fps, width, height):
        self.width, self.height = int(width), int(height)
        if not (0 < self.width <= 65535 and 0 < self.height <= 65535):
            raise ValueError("MjpegAviWriter: %dx%d" % (self.width, self.height))
        rate = float(fps)
        if not rate > 0:
            raise ValueError("MjpegAviWriter: fps must be positive")
        self.scale = 1000 if rate != int(rate) else 1
        self.rate = int(round(rate * self.scale))
        self.index, self.largest, self.closed = [], 0, False
        self.f = open(path, "wb")
        self.f.write(self._header(0, 0))
        self.movi_at = self.f.tell() - 4  # of the 'movi' tag: idx1 offsets count from it
        self.at = self.f.tell()

    def _header(self, frames, movi_bytes):
        w, h = self.width, self.height
        avih = struct.pack("<14I", 1000000 * self.scale // self.rate, self.largest * self.rate // self.scale, 0, 0x10, frames, 0, 1,
                           self.largest, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, frames, self.largest,
                           0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + \
            b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        idx_bytes = 8 + 16 * frames if frames else 0
        riff = 4 + len(hdrl) + 8 + 4 + movi_bytes + idx_bytes
        return b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"

    def write(self, data):
        if self.closed:
            raise ValueError("MjpegAviWriter: write after close")
        data = bytes(data)
        size = jpeg_size(data)
        if size != (self.width, self.height):
            raise ValueError("MjpegAviWriter: a %dx%d frame in a %dx%d video" % (size + (self.width, self.height)))
        padded = len(data) + (len(data) & 1)
        if self.at + 8 + padded + 16 * (len(self.index) + 1) + 8 > AVI_LIMIT:
            raise ValueError("MjpegAviWriter: frame %d would take the file past %d bytes, the most an AVI 1.0 file holds; "
                             "start another file" % (len(self.index), AVI_LIMIT))
        self.f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (padded - len(data)))
        self.index.append((self.at - self.movi_at, len(data)))
        self.largest = max(self.largest, len(data))
        self.at += 8 + padded

    def close(self):
        if self.closed:
            return
        self.closed = True
        movi_bytes = self.at - (self.movi_at + 4)
        if self.index:
            self.f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)) +
                         b"".join(b"00dc" + struct.pack("<III", 0x10, off, size) for off, size in self.index))
        self.f.seek(0)
        self.f.write(self._header(len(self.index), movi_bytes))
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def jpeg_size(data):
    """(width, height) of a JPEG file's first frame header; ValueError when there is none."""
    p = 2
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file")
    while p + 4 <= len(data) and data[p] == 0xFF:
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if p + 9 > len(data):
                break
            return (data[p + 7] << 8) | data[p + 8], (data[p + 5] << 8) | data[p + 6]
        if m == 0xDA:
            break
        p += 2 + n
    raise ValueError("no frame header in the JPEG file")


def read_avi_frames(path):
    """The payloads of the 00dc chunks of an AVI file this writer wrote, through its idx1 index."""
    blob = open(path, "rb").read()
    movi = blob.index(b"movi")
    idx = blob.rindex(b"idx1")
    n = struct.unpack_from("<I", blob, idx + 4)[0] // 16
    frames = []
    for k in range(n):
        _, _, off, size = struct.unpack_from("<4sIII", blob, idx + 8 + 16 * k)
        frames.append(blob[movi + off + 8:movi + off + 8 + size])
    return frames
