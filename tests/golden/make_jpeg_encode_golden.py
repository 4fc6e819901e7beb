#!/usr/bin/env python3
"""Writes tests/golden/jpeg_encode_cases.npz from Pillow (libjpeg-turbo): per case of tests/jpeg_encode_cases.py Pillow's whole
file with restart_marker_rows=1, its whole file without restarts, and its quantised coefficients, read back from its file by the
package's own entropy decoder; per quality of QUANT_QUALITIES a small file whose tables the test reads; for the fixture frame
tests/golden/nus_cam_front.jpg (decoded by jpeg.decode, encoded by Pillow at q75 4:2:0 with restart_marker_rows=1) the file's
length and sha256 only.  Needs PIL and the built library; the tests need neither PIL nor this script."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import numpy as np

import jpeg_cases as jc
import jpeg_encode_cases as ec

import bevfusion_amd  # noqa: F401
from bevfusion_amd import jpeg


def main():
    out = {"names": np.array(json.dumps([c[0] for c in ec.case_list()]))}
    for name, seed, sampling, w, h, q, noise in ec.case_list():
        px = ec.pixels(seed, w, h, noise)
        sub = ec.SAMPLING[sampling]
        rows1 = jc.encode(px, q, sub, restart_marker_rows=1)
        rows0 = jc.encode(px, q, sub)
        _, coef = jpeg.entropy_decode(rows1)
        assert np.array_equal(coef, jpeg.entropy_decode(rows0)[1])
        out[name + "_rows1"] = np.frombuffer(rows1, np.uint8)
        out[name + "_rows0"] = np.frombuffer(rows0, np.uint8)
        out[name + "_coef"] = coef
    for q in ec.QUANT_QUALITIES:
        out["quant_q%d_file" % q] = np.frombuffer(jc.encode(jc.picture(q, 8, 8), q, 2), np.uint8)
    frame = jpeg.decode(open(jc.FIXTURE, "rb").read())
    data = jc.encode(frame, ec.FIXTURE_QUALITY, 2, restart_marker_rows=1)
    out["fixture_length"] = np.array(len(data))
    out["fixture_sha256"] = np.array(hashlib.sha256(data).hexdigest())
    np.savez_compressed(ec.NPZ, **out)
    print("%s: %d bytes" % (ec.NPZ, os.path.getsize(ec.NPZ)))


if __name__ == "__main__":
    main()
