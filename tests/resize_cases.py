"""The images and sizes the resizing tests share (tests/test_resize_reference.py, tests/golden/make_resize_pins.py): every case is
named by its source, its output size and its filter, so that a pin of tests/golden/resize_pins.json can be made again on any
machine without Pillow."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
if ROOT not in sys.path:
    sys.path.append(ROOT)   # (the package, for a run of make_resize_pins.py outside pytest)

FILTERS = ("box", "bilinear", "bicubic")
IN_SIZES = [(1, 1), (2, 3), (5, 7), (17, 9), (53, 45), (64, 48), (97, 51), (100, 37), (480, 320)]   # w x h
GOLDEN_FILES = ("mini.jpg", "Mouse480.jpg")


def out_sizes(w, h):
    """1 x 1, 2 x 2, 8 x 8, 31 x 17, 224 x 224, the same size, one axis the same (each way), 2x and 3x"""
    sizes = [(1, 1), (2, 2), (8, 8), (31, 17), (224, 224), (w, h), (w, 8 if h != 8 else 9), (8 if w != 8 else 9, h), (2 * w, 2 * h), (3 * w, 3 * h)]
    return list(dict.fromkeys(sizes))   # (a 1 x 1 source: some of these coincide)


def noise(w, h, c=3):
    shape = (h, w, c) if c else (h, w)
    return np.random.default_rng(1000003 * w + 1009 * h + c).integers(0, 256, size=shape, dtype=np.uint8)


def checkerboard(w, h):
    """0 / 255 in squares of 4 x 4: bicubic overshoots at every edge, so both sides of the clip are taken"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat(((((xx >> 2) + (yy >> 2)) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def golden_rgb(name):
    """a golden file's RGB image by the library's host reader and the numpy definition of the libjpeg decode: no GPU, no Pillow"""
    import libjpeg_files as lf
    import libjpeg_reference as lj
    from video_coding_amd import hvc
    with open(os.path.join(ROOT, "tests", "golden", name), "rb") as f:
        info, coefs = hvc.jpeg_entropy_decode(f.read())
    return lj.record_to_rgb(coefs, info.qtab_array(), lf.planes_of_info(info), lf.sampling_of_info(info), info.width, info.height)


def sources():
    """name -> image, every source of the pinned cases"""
    out = {}
    for w, h in IN_SIZES:
        out["noise%dx%d" % (w, h)] = noise(w, h)
    out["grey53x45"] = noise(53, 45, 0)
    out["zeros17x9"] = np.zeros((9, 17, 3), dtype=np.uint8)
    out["ones17x9"] = np.full((9, 17, 3), 255, dtype=np.uint8)
    out["checker53x45"] = checkerboard(53, 45)
    for name in GOLDEN_FILES:
        out[name] = golden_rgb(name)
    return out


def cases(srcs):
    """(pin name, source name, W, H, filter) of every pinned case"""
    out = []
    for name, img in srcs.items():
        h, w = img.shape[:2]
        sizes = out_sizes(w, h)
        if name in GOLDEN_FILES:
            sizes = [(224, 224), (31, 17), (w // 2, h // 2), (w, 100)]
        filters = ("bicubic",) if name.startswith("checker") else FILTERS
        for W, H in sizes:
            for f in filters:
                out.append(("%s->%dx%d:%s" % (name, W, H, f), name, W, H, f))
    return out


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
