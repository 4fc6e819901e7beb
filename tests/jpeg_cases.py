"""Shared by tests/golden/make_jpeg_golden.py and the JPEG tests: the seeded picture generator, the list of recorded
streams of tests/golden/jpeg_cases.npz and the malformed variants of a stream."""
import io
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPZ = os.path.join(GOLDEN, "jpeg_cases.npz")
FIXTURE = os.path.join(GOLDEN, "nus_cam_front.jpg")

SIZES = {2: [(17, 23), (33, 9), (16, 16), (1, 1)], 1: [(19, 10)], 0: [(9, 7)]}  # Pillow's subsampling -> (W, H)
QUALITIES = (30, 75, 100)
SAMPLING_NAME = {0: "444", 1: "422", 2: "420"}


def picture(seed, w, h):
    """uint8 [h, w, 3]: seeded noise mixed with smooth gradients."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 255.0 / max(w + h - 2, 1)], -1)
    noise = rs.randint(0, 256, (h, w, 3))
    return np.clip(0.6 * base + 0.4 * noise, 0, 255).astype(np.uint8)


def encode(pixels, quality, subsampling, **kw):
    """Pillow's JPEG of the picture (needs PIL)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))


def synthetic_specs():
    """(name, seed, w, h, subsampling, quality, extra keywords) of every recorded synthetic stream."""
    specs, seed = [], 0
    for sub, sizes in SIZES.items():
        for (w, h) in sizes:
            for q in QUALITIES:
                specs.append(("%s_%dx%d_q%d" % (SAMPLING_NAME[sub], w, h, q), seed, w, h, sub, q, {}))
                seed += 1
    specs.append(("420_17x23_q75_optimize", seed, 17, 23, 2, 75, dict(optimize=True)))
    specs.append(("420_17x23_q75_restart", seed + 1, 17, 23, 2, 75, dict(restart_marker_blocks=2)))
    return specs


def random_specs():
    """The on-the-fly streams of the CPU test: every size from 1x1 to 40x40 step 3 on the diagonal and two off it, cycling
    the sampling modes and qualities."""
    specs = []
    sizes = list(range(1, 41, 3))
    for i, w in enumerate(sizes):
        for h in (w, sizes[(i * 5 + 3) % len(sizes)], sizes[(i * 3 + 7) % len(sizes)]):
            k = len(specs)
            specs.append((1000 + k, w, h, k % 3, QUALITIES[(k // 3) % 3], dict(optimize=True) if k % 4 == 1 else {}))
    return specs


_cases = None


def load():
    """The npz as a dict, read once."""
    global _cases
    if _cases is None:
        with np.load(NPZ) as z:
            _cases = {k: z[k] for k in z.files}
    return _cases


def streams():
    """[(name, bytes, recorded Pillow pixels uint8 [h, w, 3])] of section (a)."""
    z = load()
    names = json.loads(str(z["stream_names"]))
    return [(n, z["stream_%s_bytes" % n].tobytes(), z["stream_%s_pixels" % n]) for n in names]


def unsupported_streams():
    z = load()
    return [(n, z["unsupported_%s_bytes" % n].tobytes()) for n in json.loads(str(z["unsupported_names"]))]


def malformed(data, seed):
    """The variants of one stream: 16 evenly spaced truncations, then 32 seeded single-byte corruptions."""
    data = bytes(data)
    out = [data[:len(data) * k // 17] for k in range(1, 17)]
    rs = np.random.RandomState(seed)
    for _ in range(32):
        b = bytearray(data)
        b[rs.randint(0, len(b))] = rs.randint(0, 256)
        out.append(bytes(b))
    return out
