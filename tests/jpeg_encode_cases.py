"""Shared by tests/golden/make_jpeg_encode_golden.py and the JPEG encoder tests: the recorded cases of
tests/golden/jpeg_encode_cases.npz and the hand-made and seeded coefficient sets of the entropy-stage tests."""
import json
import os

import numpy as np

import jpeg_cases as jc

NPZ = os.path.join(jc.GOLDEN, "jpeg_encode_cases.npz")
SAMPLING = {"4:2:0": 2, "4:2:2": 1, "4:4:4": 0}  # -> Pillow's subsampling
ALL_Q = (30, 75, 100)
# (sampling, W, H, qualities, noise): the smallest sizes at which each rule of the encoder can go wrong
CASES = [
    ("4:2:0", 1, 1, ALL_Q, False),      # everything is padding; three of four luma blocks are dummies
    ("4:2:0", 16, 16, ALL_Q, False),    # a whole MCU, no padding
    ("4:2:0", 17, 23, ALL_Q, False),    # partial in both directions; dummy column and dummy row together
    ("4:2:0", 33, 9, ALL_Q, False),     # dummy bottom block row only
    ("4:2:0", 22, 31, ALL_Q, False),    # even / odd H difference of the bottom extension
    ("4:2:0", 40, 150, (75,), False),   # 10 intervals: the RST numbering wraps
    ("4:2:0", 700, 16, (100,), True),   # 264 blocks in one interval, over 100 stuffed bytes, categories 9-10
    ("4:2:0", 64, 64, (5,), False),     # almost every block is DC + EOB
    ("4:2:2", 19, 10, ALL_Q, False),    # h2v1 bias and its dummy column
    ("4:4:4", 9, 7, ALL_Q, False),      # no subsampling
]
QUANT_QUALITIES = (1, 10, 49, 50, 51, 75, 95, 100)
FIXTURE_QUALITY = 75


def case_list():
    """[(name, seed, sampling, w, h, quality, noise)]"""
    out = []
    for k, (sampling, w, h, qualities, noise) in enumerate(CASES):
        for q in qualities:
            out.append(("%s_%dx%d_q%d" % (sampling.replace(":", ""), w, h, q), 5000 + 10 * k, sampling, w, h, q, noise))
    return out


def pixels(seed, w, h, noise):
    """uint8 [h, w, 3]: jpeg_cases.picture, or uniform noise."""
    if noise:
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    return jc.picture(seed, w, h)


_cases = None


def load():
    global _cases
    if _cases is None:
        with np.load(NPZ) as z:
            _cases = {k: z[k] for k in z.files}
    return _cases


def recorded():
    """[(name, seed, sampling, w, h, quality, noise, Pillow's file with restart_marker_rows=1, Pillow's file without restarts,
    Pillow's coefficients int16)]"""
    z = load()
    assert json.loads(str(z["names"])) == [c[0] for c in case_list()]
    return [c + (z[c[0] + "_rows1"].tobytes(), z[c[0] + "_rows0"].tobytes(), z[c[0] + "_coef"]) for c in case_list()]


# ---------------------------------------------------------------------------------------------- coefficient sets
def _header(jpeg, w, h, hs, vs):
    return jpeg.make_header(w, h, hs, vs, np.ones((3, 64), np.uint16))


def _blocks(header, coef, c):
    n = header.block_rows[c] * header.block_cols[c]
    return coef[header.coef_offset[c]:header.coef_offset[c] + n * 64].reshape(header.block_rows[c], header.block_cols[c], 64)


ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def coefficient_sets(jpeg):
    """[(name, Header, int16 coefficients)]: legal coefficients that did not come from a picture.  `jpeg`: bevfusion_amd.jpeg."""
    sets = []
    for name, value in (("ac_plus_1023", 1023), ("ac_minus_1023", -1023)):
        h = _header(jpeg, 16, 16, 2, 2)
        coef = np.full(h.coef_bytes // 2, value, np.int16)
        coef[0::64] = 0
        sets.append((name, h, coef))
    # zero runs of exactly 15, 16, 17, 32 and 48 before a non-zero value (also after a first value), and a non-zero coefficient 63
    h = _header(jpeg, 48, 16, 1, 1)
    coef = np.zeros(h.coef_bytes // 2, np.int16)
    for c in range(3):
        blocks = _blocks(h, coef, c).reshape(-1, 64)
        for b, run in enumerate((15, 16, 17, 32, 48)):
            blocks[b, ZIGZAG[1 + run]] = 3 + b           # `run` zeros from position 1 on
            if 2 + 2 * run < 64:
                blocks[b, ZIGZAG[2 + 2 * run]] = -7      # and `run` more
        blocks[5, ZIGZAG[63]] = -2                        # no EOB
        blocks[6, ZIGZAG[62]] = 1
        blocks[7, ZIGZAG[63]] = 1023
        blocks[7, ZIGZAG[1]] = -1
        blocks[:, 0] = np.arange(len(blocks)) * 5 - 20
    sets.append(("runs", h, coef))
    # DC steps of +2047 and -2047 between neighbours, in every component
    h = _header(jpeg, 40, 8, 1, 1)
    coef = np.zeros(h.coef_bytes // 2, np.int16)
    for c in range(3):
        _blocks(h, coef, c)[0, :, 0] = [-1000, 1047, -1000, 1023, -1024]
    sets.append(("dc_steps", h, coef))
    # 16 bits: luma DC 1 (3 + 1 bits) and its EOB (4), two chroma blocks of DC 0 (2) and EOB (2): no padding bits
    h = _header(jpeg, 8, 8, 1, 1)
    coef = np.zeros(h.coef_bytes // 2, np.int16)
    coef[0] = 1
    sets.append(("byte_aligned", h, coef))
    # seeded: sparse blocks with magnitudes of every category; the last is wider than a 256-thread workgroup (270 blocks an interval)
    rs = np.random.RandomState(11)
    for name, (w, h_, hs, vs) in (("random_420", (40, 37, 2, 2)), ("random_422", (35, 17, 2, 1)), ("random_444", (21, 20, 1, 1)),
                                  ("random_wide", (716, 24, 2, 2))):
        h = _header(jpeg, w, h_, hs, vs)
        n = h.coef_bytes // 2
        mag = (2.0 ** rs.uniform(0, 10, n)).astype(np.int64).clip(1, 1023)
        coef = (mag * rs.choice([-1, 1], n) * (rs.uniform(size=n) < rs.choice([0.02, 0.15, 0.6], n // 64).repeat(64))).astype(np.int16)
        coef[0::64] = rs.randint(-1023, 1025, n // 64)
        if name == "random_444":
            coef[0::64] = rs.choice([-1023, 1024], n // 64)   # only steps of 0 and +-2047
            coef.reshape(-1, 64)[::3, 1:] = 255                # bytes of FF
        sets.append((name, h, coef))
    return sets
