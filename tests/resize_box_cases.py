"""The boxes, sizes and images the box / mirror / typed-output tests share (tests/test_resize_box_reference.py,
tests/golden/make_resize_box_pins.py, tests/test_gpu_resize_box.py): every case is named by its source, its output size, its
filter, its box and its mirror flag, so that a pin of tests/golden/resize_box_pins.json can be made again on any machine
without Pillow."""
import numpy as np

import resize_cases as rc

FILTERS = rc.FILTERS
IN_SIZES = [(1, 1), (2, 3), (5, 7), (17, 9), (53, 45), (64, 48), (70, 53)]   # w x h


def f32(v):
    return float(np.float32(v))


def boxes(w, h):
    """name -> box of a w x h image: the whole image (None and spelled out), an integer box, a fractional one, one thinner than a
    pixel on both axes, and one touching each edge -- every value an IEEE single"""
    out = {"none": None, "whole": (0.0, 0.0, float(w), float(h))}
    if w >= 4 and h >= 4:
        out["integer"] = (float(w // 4), float(h // 4), float(w - w // 4), float(h - h // 3))
    out["fraction"] = (f32(w * 0.13), f32(h * 0.21), f32(w * 0.87), f32(h * 0.77))
    out["thin"] = (f32(w * 0.5), f32(h * 0.4), f32(w * 0.5 + 0.25), f32(h * 0.4 + 0.3))
    out["left"] = (0.0, f32(h * 0.3), f32(w * 0.6), f32(h * 0.9))
    out["top"] = (f32(w * 0.2), 0.0, f32(w * 0.7), f32(h * 0.55))
    out["right"] = (f32(w * 0.35), f32(h * 0.1), float(w), f32(h * 0.8))
    out["bottom"] = (f32(w * 0.1), f32(h * 0.45), f32(w * 0.95), float(h))
    return out


def out_sizes(w, h):
    """1 x 1, 31 x 17 (down and up), the same size (only a whole box skips an axis), and 2x"""
    return list(dict.fromkeys([(1, 1), (31, 17), (w, h), (2 * w, 2 * h)]))


def sources():
    """the pinned sources: RGB noise from 1 x 1 to 53 x 45, and one grey (mode L) image"""
    out = {"noise%dx%d" % (w, h): rc.noise(w, h) for w, h in ((1, 1), (5, 7), (17, 9), (53, 45))}
    out["grey53x45"] = rc.noise(53, 45, 0)
    return out


def cases(srcs):
    """(pin name, source name, W, H, filter, box, mirror) of every pinned case: every source at every size under every kind of
    box -- at 31 x 17 under the three filters, elsewhere under one, taken in turn; the mirror flag alternates, so that every
    kind of box meets both"""
    out, k = [], 0
    for name, img in srcs.items():
        h, w = img.shape[:2]
        for si, (W, H) in enumerate(out_sizes(w, h)):
            for bi, (bname, box) in enumerate(boxes(w, h).items()):
                for f in (FILTERS if (W, H) == (31, 17) else (FILTERS[(si + bi) % 3],)):
                    mirror = bool(k & 1)
                    k += 1
                    out.append(("%s>%dx%d %s %s m%d" % (name, W, H, f, bname, mirror), name, W, H, f, box, mirror))
    return out


sha256 = rc.sha256
