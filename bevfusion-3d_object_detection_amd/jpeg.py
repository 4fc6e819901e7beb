"""JPEG decode split at the entropy stage (csrc/jpeg_host.h, csrc/jpeg.hip).

A baseline JPEG decode has a serial half -- the Huffman (entropy) stage -- and a data-parallel half: dequantisation, the 8x8
inverse DCT, chroma upsampling and YCbCr -> RGB.  `parse` and `entropy_decode` run the first on the host (bfhip_jpeg_parse,
bfhip_jpeg_entropy_decode: plain C++, no HIP call, the GIL released: safe in a loader's worker, which never opens the device)
and leave per component [block_rows, block_cols, 64] int16 coefficients in natural order, DC prediction undone, not dequantised.

`torch_jpeg_decode(header, coef)` is the second half in numpy int32 and DEFINES the device stage: libjpeg's accurate integer
IDCT (jidctint: CONST_BITS 13, PASS1_BITS 2; column pass first, descaled by 11, row pass by 18, + 128, clamp), its "fancy"
triangle-filter upsampling (neighbours outside the component's real extent ceil(W / h) x ceil(H / v) are the nearest real
sample; a component of at most two samples a row is replicated instead, as libjpeg chooses) and its 16-bit fixed-point colour
conversion.  Every sum and product is 32-bit two's-complement wrap-around, so it is defined on every int16 input.  On what an
encoder writes it equals Pillow's decode bit for bit (tests/test_jpeg_cpu.py).

`JpegFrames` is what BEVLoadMultiViewImageFromFiles(defer=True) leaves in data["img"]: the frames' headers and ONE int16
coefficient buffer, nothing decoded.  `decode_frames` turns a list of them into the uint8 [N, H, W, 3] blocks on a device:
`fused_jpeg_decode` (bfhip_jpeg_decode: one pinned upload -- coefficients and descriptor table -- and two launches for the
whole batch) or, with BFHIP_JPEG_DECODE=0 or on the CPU, the restatement.  Same bits either way.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib

ENABLED = os.environ.get("BFHIP_JPEG_DECODE", "1") != "0"
PATHS = {"kernel": 0, "torch": 0}  # batches decoded by each path (tests, tools)

REASONS = {0: "supported", 1: "progressive", 2: "arithmetic coding", 3: "not 8 bits per sample", 4: "not three components",
           5: "more than one scan", 6: "16-bit quantisation table", 7: "sampling factors", 8: "EXIF orientation tag",
           9: "not baseline sequential", 10: "not YCbCr"}


class Header(ctypes.Structure):
    """bfhip_jpeg_header (include/bevfusion_hip.h)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32),
                ("supported", ctypes.c_int32), ("reason", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("mcus_x", ctypes.c_int32), ("mcus_y", ctypes.c_int32), ("hs", ctypes.c_int32 * 3), ("vs", ctypes.c_int32 * 3),
                ("block_cols", ctypes.c_int32 * 3), ("block_rows", ctypes.c_int32 * 3), ("coef_offset", ctypes.c_int64 * 3),
                ("coef_bytes", ctypes.c_int64), ("quant", (ctypes.c_uint16 * 64) * 3)]

    def quant_array(self):
        return np.ctypeslib.as_array(self.quant).reshape(3, 64).copy()


class _Frame(ctypes.Structure):
    """bfhip_jpeg_frame (include/bevfusion_hip.h)."""
    _fields_ = [("coef_off", ctypes.c_int64 * 3), ("plane_off", ctypes.c_int64 * 3), ("rgb_off", ctypes.c_int64),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("hs", ctypes.c_int32), ("vs", ctypes.c_int32),
                ("block_cols", ctypes.c_int32 * 3), ("block_rows", ctypes.c_int32 * 3), ("quant", (ctypes.c_uint16 * 64) * 3)]


def make_header(width, height, hs, vs, quant):
    """A header for coefficients that did not come from a file (tests, tools): luma sampling hs x vs, chroma 1x1, quant uint16
    [3, 64] in natural order."""
    h = Header()
    h.width, h.height, h.ncomp, h.supported = int(width), int(height), 3, 1
    h.mcus_x, h.mcus_y = -(-h.width // (8 * hs)), -(-h.height // (8 * vs))
    off = 0
    for c in range(3):
        h.hs[c], h.vs[c] = (hs, vs) if c == 0 else (1, 1)
        h.block_cols[c], h.block_rows[c] = h.mcus_x * h.hs[c], h.mcus_y * h.vs[c]
        h.coef_offset[c] = off
        off += h.block_cols[c] * h.block_rows[c] * 64
        for i in range(64):
            h.quant[c][i] = int(quant[c][i])
    h.coef_bytes = off * 2
    return h


def _as_bytes(data):
    data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data)
    if data.dtype != np.uint8 or data.ndim != 1:
        raise TypeError("a JPEG stream must be bytes or a uint8 vector")
    return np.ascontiguousarray(data)


def parse(data):
    """bfhip_jpeg_parse: the Header of a stream; RuntimeError when the stream is malformed.  header.supported tells whether
    the fused decoder takes it (header.reason: REASONS)."""
    data = _as_bytes(data)
    h = Header()
    _lib.call("bfhip_jpeg_parse", data.ctypes.data, data.size, ctypes.addressof(h))
    return h


def supported(data):
    """True when the fused decoder takes this stream (False for a malformed one as well)."""
    try:
        return bool(parse(data).supported)
    except RuntimeError:
        return False


def entropy_decode(data, header=None, out=None):
    """bfhip_jpeg_entropy_decode: (header, int16 coefficients [header.coef_bytes / 2]).  `out`: an int16 vector to write into."""
    data = _as_bytes(data)
    header = parse(data) if header is None else header
    if not header.supported:
        raise RuntimeError("jpeg: the fused decoder does not take this stream (%s)" % REASONS.get(header.reason, header.reason))
    coef = np.empty(header.coef_bytes // 2, dtype=np.int16) if out is None else out
    _lib.call("bfhip_jpeg_entropy_decode", data.ctypes.data, data.size, ctypes.addressof(header), coef.ctypes.data, coef.nbytes)
    return header, coef


# ---------------------------------------------------------------------------------------------- the restatement
def _idct_pass(v, shift):
    """One pass of jidctint's 8-point inverse DCT along the last axis of an int32 array, wrap-around, descaled by `shift`."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k] for k in range(8))
    c = np.int32
    z1 = (i2 + i6) * c(4433)
    e2 = z1 + i6 * c(-15137)
    e3 = z1 + i2 * c(6270)
    e0, e1 = (i0 + i4) << c(13), (i0 - i4) << c(13)
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    o0, o1, o2, o3 = i7, i5, i3, i1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * c(9633)
    o0, o1, o2, o3 = o0 * c(2446), o1 * c(16819), o2 * c(25172), o3 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    o0, o1, o2, o3 = o0 + (z1 + z3), o1 + (z2 + z4), o2 + (z2 + z3), o3 + (z1 + z4)
    half = c(1 << (shift - 1))
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([(x + half) >> c(shift) for x in out], -1)


def _planes(header, coef):
    """The three uint8 component planes, whole blocks: [block_rows * 8, block_cols * 8] each."""
    coef = np.asarray(coef).reshape(-1)
    if coef.dtype != np.int16 or coef.size * 2 < header.coef_bytes:
        raise ValueError("coef must be int16 with at least %d values" % (header.coef_bytes // 2))
    planes = []
    with np.errstate(over="ignore"):
        for c in range(3):
            br, bc = header.block_rows[c], header.block_cols[c]
            blocks = coef[header.coef_offset[c]:header.coef_offset[c] + br * bc * 64].reshape(br, bc, 8, 8).astype(np.int32)
            q = np.ctypeslib.as_array(header.quant[c]).astype(np.int32).reshape(8, 8)
            x = blocks * q
            x = _idct_pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)  # columns first
            x = _idct_pass(x, 18)
            x = np.clip(x + np.int32(128), 0, 255).astype(np.uint8)
            planes.append(np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(br * 8, bc * 8))
    return planes


def _upsample(plane, W, H, hs, vs):
    """libjpeg's upsampling of one chroma plane to int32 [H, W]; the plane is first cut to its real extent."""
    cw, ch = -(-W // hs), -(-H // vs)
    p = plane[:ch, :cw].astype(np.int32)
    x, y = np.arange(W), np.arange(H)
    if hs == 1 and vs == 1:
        return p
    if hs == 2 and cw <= 2:  # too narrow for the triangle filter: replicated, rows as well
        return p[(y >> 1) if vs == 2 else y][:, x >> 1]
    if hs == 2:
        cx, oddx = x >> 1, x & 1
        nbx = np.where(oddx == 1, np.minimum(cx + 1, cw - 1), np.maximum(cx - 1, 0))
    if vs == 1:
        return (3 * p[:, cx] + p[:, nbx] + np.where(oddx == 1, 2, 1)) >> 2
    cy, oddy = y >> 1, y & 1
    fy = np.where(oddy == 1, np.minimum(cy + 1, ch - 1), np.maximum(cy - 1, 0))
    if hs == 1:
        return (3 * p[cy] + p[fy] + np.where(oddy == 1, 2, 1)[:, None]) >> 2
    colsum = 3 * p[cy] + p[fy]  # [H, cw]
    return (3 * colsum[:, cx] + colsum[:, nbx] + np.where(oddx == 1, 7, 8)) >> 4


def torch_jpeg_decode(header, coef):
    """header (Header) + int16 coefficients (numpy or torch, as entropy_decode leaves them) -> uint8 tensor [H, W, 3] (CPU)."""
    if torch.is_tensor(coef):
        coef = coef.cpu().numpy()
    W, H, hs, vs = header.width, header.height, header.hs[0], header.vs[0]
    if hs not in (1, 2) or vs not in (1, 2) or any(header.hs[c] != 1 or header.vs[c] != 1 for c in (1, 2)):
        raise ValueError("sampling %s x %s is not supported" % (list(header.hs), list(header.vs)))
    luma, cb, cr = _planes(header, coef)
    y = luma[:H, :W].astype(np.int32)
    b = (_upsample(cb, W, H, hs, vs) - 128).astype(np.int32)
    r = (_upsample(cr, W, H, hs, vs) - 128).astype(np.int32)
    c = np.int32
    rgb = np.stack([y + ((c(91881) * r + c(32768)) >> c(16)),
                    y + ((c(-22554) * b + c(-46802) * r + c(32768)) >> c(16)),
                    y + ((c(116130) * b + c(32768)) >> c(16))], -1)
    return torch.from_numpy(np.clip(rgb, 0, 255).astype(np.uint8))


def decode(data):
    """A whole stream through this package's decoder on the host: uint8 array [H, W, 3]."""
    header, coef = entropy_decode(data)
    return torch_jpeg_decode(header, coef).numpy()


# ---------------------------------------------------------------------------------------------- deferred frames
class JpegFrames:
    """The entropy-decoded frames of one sample: `headers` (one Header per frame), `coef` (ONE int16 vector, the frames'
    coefficient buffers end to end) and `offsets` (int16 elements, len(headers) + 1).  shape = (N, H, W, 3) of the decoded
    block; frames smaller than the largest are zero-padded at the bottom and right, as the loader pads decoded frames."""

    def __init__(self, headers, coef, offsets):
        self.headers, self.coef, self.offsets = list(headers), coef, [int(o) for o in offsets]
        if len(self.offsets) != len(self.headers) + 1 or not self.headers:
            raise ValueError("JpegFrames: %d offsets for %d headers" % (len(self.offsets), len(self.headers)))
        self.shape = (len(self.headers), max(h.height for h in self.headers), max(h.width for h in self.headers), 3)

    @classmethod
    def from_bytes(cls, streams):
        """The entropy stage of every stream, into one buffer.  RuntimeError when a stream is malformed or not supported."""
        streams = [_as_bytes(s) for s in streams]
        headers = [parse(s) for s in streams]
        for h in headers:
            if not h.supported:
                raise RuntimeError("jpeg: the fused decoder does not take this stream (%s)" % REASONS.get(h.reason, h.reason))
        offsets = np.concatenate([[0], np.cumsum([h.coef_bytes // 2 for h in headers])])
        coef = np.empty(int(offsets[-1]), dtype=np.int16)
        for s, h, lo, hi in zip(streams, headers, offsets[:-1], offsets[1:]):
            entropy_decode(s, h, coef[lo:hi])
        return cls(headers, coef, offsets)

    def __len__(self):
        return len(self.headers)

    def frame(self, i):
        return self.headers[i], self.coef[self.offsets[i]:self.offsets[i + 1]]

    def padded(self):
        """True when the frames differ in size (the decoded block then has zero padding)."""
        return any((h.height, h.width) != self.shape[1:3] for h in self.headers)

    def decode_host(self):
        """The restatement: uint8 tensor [N, H, W, 3] on the CPU."""
        out = torch.zeros(self.shape, dtype=torch.uint8)
        for i in range(len(self)):
            h, coef = self.frame(i)
            out[i, :h.height, :h.width] = torch_jpeg_decode(h, coef)
        return out


def fused_decode_batch(frames, device, planes=None, guard=0):
    """frames: list of (Header, int16 coefficient vector) -> (list of uint8 [h, w, 3] tensors on `device`, the flat buffer they
    are views of).  One pinned host-to-device copy (every frame's coefficients, the descriptor table behind them) and
    bfhip_jpeg_decode's two launches for the whole batch, whatever the frames' sizes, sampling and tables; no synchronisation.
    Frames follow one another densely in the buffer.  planes: a preallocated uint8 device buffer for the component planes;
    guard: spare bytes of 0xA5 behind the last frame (tests)."""
    device = torch.device(device)
    n = len(frames)
    sizes = [h.coef_bytes // 2 for h, _ in frames]
    coef_elems = int(sum(sizes))
    table_at = (coef_elems * 2 + 15) // 16 * 16
    staging = torch.empty(table_at + ctypes.sizeof(_Frame) * n, dtype=torch.uint8).pin_memory()
    host = staging.numpy()
    descs = (_Frame * n).from_buffer(host[table_at:])
    coef_at = plane_at = rgb_at = 0
    views = []
    for d, (h, coef), size in zip(descs, frames, sizes):
        coef = np.asarray(coef).reshape(-1)
        if coef.dtype != np.int16 or coef.size < size:
            raise ValueError("fused_decode_batch: coefficients must be int16 with %d values" % size)
        host[coef_at * 2:(coef_at + size) * 2] = coef[:size].view(np.uint8)
        d.width, d.height, d.hs, d.vs = h.width, h.height, h.hs[0], h.vs[0]
        for c in range(3):
            d.coef_off[c] = coef_at + h.coef_offset[c]
            d.plane_off[c] = plane_at
            d.block_cols[c], d.block_rows[c] = h.block_cols[c], h.block_rows[c]
            plane_at += h.block_cols[c] * h.block_rows[c] * 64
        ctypes.memmove(d.quant, h.quant, ctypes.sizeof(h.quant))
        d.rgb_off = rgb_at
        views.append((rgb_at, (h.height, h.width, 3)))
        coef_at += size
        rgb_at += h.height * h.width * 3
    on_dev = staging.to(device, non_blocking=True)  # the batch's one upload
    if planes is None:
        planes = torch.empty(plane_at, dtype=torch.uint8, device=device)
    if planes.numel() < plane_at or planes.dtype != torch.uint8 or not planes.is_contiguous() or planes.device != device:
        raise ValueError("fused_decode_batch: planes does not hold %d bytes on %s" % (plane_at, device))
    rgb = torch.empty(rgb_at + guard, dtype=torch.uint8, device=device)
    if guard:
        rgb[rgb_at:] = 0xA5
    with torch.cuda.device(device):
        _lib.call("bfhip_jpeg_decode", ctypes.addressof(descs), on_dev.data_ptr() + table_at, n, on_dev.data_ptr(), coef_elems,
                  planes.data_ptr(), planes.numel(), rgb.data_ptr(), rgb_at, _lib.stream_of(rgb))
    return [rgb[at:at + shape[0] * shape[1] * 3].view(shape) for at, shape in views], rgb


def fused_jpeg_decode(samples, device, planes=None):
    """samples: list of JpegFrames whose frames have one size per sample -> list of uint8 [N, H, W, 3] tensors on `device`,
    views of one buffer: fused_decode_batch over every frame of the batch."""
    if any(s.padded() for s in samples):
        raise ValueError("fused_jpeg_decode: a sample's frames differ in size")
    frames = [s.frame(i) for s in samples for i in range(len(s))]
    _, rgb = fused_decode_batch(frames, device, planes)
    out, at = [], 0
    for s in samples:
        size = int(np.prod(s.shape))
        out.append(rgb[at:at + size].view(s.shape))
        at += size
    return out


def decode_frames(samples, device):
    """list of JpegFrames -> list of uint8 [N, H, W, 3] tensors on `device`: the fused path on a GPU (BFHIP_JPEG_DECODE, ships
    on), the restatement otherwise -- also for a sample whose frames differ in size, which is zero-padded on the host."""
    device = torch.device(device)
    if ENABLED and device.type == "cuda" and not any(s.padded() for s in samples):
        PATHS["kernel"] += 1
        return fused_jpeg_decode(samples, device)
    PATHS["torch"] += 1
    return [s.decode_host().to(device) for s in samples]
