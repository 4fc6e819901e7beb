#!/usr/bin/env python3
"""Writes tests/golden/grid_mask.npz: the reference's own GridMask (numpy canvas, PIL rotate) on seeded float32 frames, for
tests/test_grid_mask_cpu.py.

The reference's transforms_3d.py is loaded at run time from REFERENCE_ROOT, as make_image_aug_golden.py loads it and behind the
same stubs; nothing of it is copied.  Needs PIL.

Two frame sets, integer-valued float32 in 1 .. 255 (so that the mask can be read off the output): "a" 3 cameras of 16 x 40 and
"b" 2 cameras of 20 x 20.  Cases: every combination of mode 0 / 1, use_h / use_w alone and together, ratio 0.5 / 1 and rotate
1 / 360 once on each set with its own seed; prob 0.0, 0.6 and 1.0 with fixed_prob; fixed_prob=False with set_epoch(3) of
max_epoch=6; and cases whose seed is the first one for which the reference draws what the tests need (searched here, asserted
below): r = 0 and r in 90 / 180 / 270 out of rotate=360 on the square set, a rotated canvas that leaves part of the window
outside in both modes, and an unrotated draw where a row or column beyond the last of the size // d bands stays unmasked although
a periodic rule would mask it.  Per case: the keywords, seed and epoch, whether the mask was applied, the integers the reference
drew (np.random.randint is wrapped by a recorder for the call), the mask, the output frames and the next np.random.uniform()."""
import importlib.util
import json
import os

import numpy as np
from PIL import Image

from make_image_aug_golden import REF, load_reference

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = {"a": (3, 16, 40), "b": (2, 20, 20)}
BASE = dict(use_h=True, use_w=True, max_epoch=6, rotate=1, offset=False, ratio=0.5, mode=0, prob=1.0, fixed_prob=True)


def load_grid_mask():
    load_reference()  # installs the stubs (and returns the module's ImageAug3D, which is not needed here)
    spec = importlib.util.spec_from_file_location("reference_transforms_3d", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.GridMask


def frames_of(key):
    n, h, w = SETS[key]
    return np.random.RandomState(77 + ord(key)).randint(1, 256, (n, h, w, 3)).astype(np.float32)


def run(cls, key, cfg, seed, epoch=None):
    """One call of the reference's transform -> dict of what is recorded."""
    aug = cls(**cfg)
    if epoch is not None:
        aug.set_epoch(epoch)
    frames = frames_of(key)
    drawn, real = [], np.random.randint

    def recorder(*a, **k):
        drawn.append(int(real(*a, **k)))
        return drawn[-1]

    np.random.seed(seed)
    np.random.randint = recorder
    try:
        res = aug.transform(dict(img=[f.copy() for f in frames]))
    finally:
        np.random.randint = real
    nxt = np.random.uniform()
    out = np.stack([np.asarray(x, dtype=np.float32) for x in res["img"]])
    applied = len(drawn) > 0
    n, h, w = SETS[key]
    if applied:
        assert len(drawn) == (5 if cfg["ratio"] == 1 else 4), drawn
        d, st_h, st_w, r = drawn[0], drawn[-3], drawn[-2], drawn[-1]
        ints = [d, int(aug.length), st_h, st_w, r]
        mask = (out[0, :, :, 0] != 0)
        assert all(np.array_equal(out[c], frames[c] * mask[:, :, None].astype(np.float32)) for c in range(n))
    else:
        ints, mask = [0, 0, 0, 0, 0], np.ones((h, w), bool)
        assert np.array_equal(out, frames)
    assert np.array_equal(out, out.astype(np.uint8))
    return dict(set=key, cfg=cfg, seed=seed, epoch=-1 if epoch is None else epoch, applied=applied, ints=ints,
                mask=mask.astype(np.uint8), out=out.astype(np.uint8), next_uniform=nxt)


def has_fill(case):
    """Part of the window lies outside the rotated canvas (PIL alone: an all-ones canvas, rotated and cropped)."""
    _, h, w = SETS[case["set"]]
    hh, ww = int(1.5 * h), int(1.5 * w)
    ones = np.asarray(Image.fromarray(np.ones((hh, ww), np.uint8)).rotate(case["ints"][4]))
    return case["applied"] and not ones[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w].all()


def beyond_last_band(case):
    """Unrotated: a window row (column) past the last of the size // d bands that a periodic rule would mask, and that is 1."""
    if not case["applied"] or case["ints"][4] != 0:
        return False
    _, h, w = SETS[case["set"]]
    d, length, st_h, st_w, _ = case["ints"]
    canvas = case["mask"] if case["cfg"]["mode"] != 1 else 1 - case["mask"]
    for use, size, win, st, lines in ((case["cfg"]["use_h"], int(1.5 * h), h, st_h, canvas),
                                      (case["cfg"]["use_w"], int(1.5 * w), w, st_w, canvas.T)):
        o = (size - win) // 2
        for v in range(o, o + win):
            t = v - st
            if use and t >= 0 and t // d >= size // d and t % d < length and lines[v - o].any():
                return True
    return False


def first_seed(cls, key, cfg, wanted, epoch=None):
    for seed in range(100000):
        case = run(cls, key, cfg, seed, epoch)
        if wanted(case):
            return case
    raise AssertionError("no seed below 100000 gives the wanted draw")


def main():
    cls = load_grid_mask()
    cases = []
    k = 0
    for mode in (0, 1):
        for use_h, use_w in ((True, False), (False, True), (True, True)):
            for ratio in (0.5, 1):
                for rotate in (1, 360):
                    cfg = dict(BASE, mode=mode, use_h=use_h, use_w=use_w, ratio=ratio, rotate=rotate)
                    cases.append(run(cls, "a", cfg, 100 + k))
                    cases.append(run(cls, "b", cfg, 200 + k))
                    k += 1
    for seed in (0, 1):
        cases.append(run(cls, "a", dict(BASE, mode=1, prob=0.0), seed))  # the shipped configuration
    for seed in range(6):
        cases.append(run(cls, "a" if seed % 2 else "b", dict(BASE, prob=0.6, rotate=360), 300 + seed))
    at06 = [c["applied"] for c in cases[-6:]]
    for seed in range(4):
        cases.append(run(cls, "b" if seed % 2 else "a", dict(BASE, fixed_prob=False, mode=seed // 2), 400 + seed, epoch=3))
    at05 = [c["applied"] for c in cases[-4:]]
    full = dict(BASE, rotate=360)
    cases.append(first_seed(cls, "b", full, lambda c: c["applied"] and c["ints"][4] == 0))
    cases.append(first_seed(cls, "b", full, lambda c: c["applied"] and c["ints"][4] in (90, 180, 270)))
    cases.append(first_seed(cls, "a", full, has_fill))
    cases.append(first_seed(cls, "a", dict(full, mode=1), has_fill))
    cases.append(first_seed(cls, "b", BASE, beyond_last_band))
    cases.append(first_seed(cls, "a", dict(BASE, use_w=False, mode=1), beyond_last_band))

    assert True in at06 and False in at06, "prob=0.6: a skipped and an applied draw are needed: %s" % at06
    assert True in at05 and False in at05, "set_epoch(3) of 6: a skipped and an applied draw are needed: %s" % at05
    assert not any(c["applied"] for c in cases if c["cfg"]["prob"] == 0.0)
    for mode in (0, 1):
        assert any(has_fill(c) for c in cases if c["cfg"]["mode"] == mode), "no fill pixels in mode %d" % mode
    assert any(beyond_last_band(c) for c in cases)
    square = [c["ints"][4] for c in cases if c["set"] == "b" and c["applied"] and c["cfg"]["rotate"] == 360]
    assert 0 in square and any(r in (90, 180, 270) for r in square), square

    out = dict(n_cases=np.array(len(cases)), frames_a=frames_of("a").astype(np.uint8), frames_b=frames_of("b").astype(np.uint8))
    for i, c in enumerate(cases):
        out["case%d_set" % i] = np.array(c["set"])
        out["case%d_cfg" % i] = np.array(json.dumps(c["cfg"], sort_keys=True))
        out["case%d_seed" % i] = np.array(c["seed"])
        out["case%d_epoch" % i] = np.array(c["epoch"])
        out["case%d_applied" % i] = np.array(c["applied"])
        out["case%d_ints" % i] = np.array(c["ints"], np.int64)  # d, length, st_h, st_w, r
        out["case%d_mask" % i] = c["mask"]
        out["case%d_out" % i] = c["out"]
        out["case%d_next_uniform" % i] = np.array(c["next_uniform"], np.float64)
    path = os.path.join(HERE, "grid_mask.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
