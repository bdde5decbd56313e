"""Writes tests/golden/resize_box_pins.json: the SHA-256 of what Pillow makes of the cases of tests/resize_box_cases.py --
Image.resize((W, H), filter, box=box), then (mirror) .transpose(FLIP_LEFT_RIGHT) -- under "sha256", and under "libjpeg_sha256"
the same of Image.open(f).convert("RGB") for the two golden files (what hvc_jpeg_decode_batch_mixed_resized_opts gives under
hvc_set_mixed_arithmetic(HVC_ARITH_LIBJPEG)).  tests/test_resize_box_reference.py regenerates and compares them where Pillow is
installed, and holds tools/resize_reference.py resize_box against them everywhere.

    python tests/golden/make_resize_box_pins.py"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_box_cases as bc  # noqa: E402

GOLDEN_FILES = ("mini.jpg", "Mouse480.jpg")
GOLDEN_SIZES = {"mini.jpg": (24, 16), "Mouse480.jpg": (31, 17)}
GOLDEN_BOXES = ("integer", "fraction", "left", "bottom")


def pillow_resize_box(img, W, H, filter, box, mirror):
    from PIL import Image
    f = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filter]
    im = img if isinstance(img, Image.Image) else Image.fromarray(img)
    out = im.resize((W, H), f, box=box)
    if mirror:
        out = out.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(out)


def golden_cases():
    """(pin name, file, W, H, filter, box, mirror): every golden file under every filter and GOLDEN_BOXES, mirrored every other
    time"""
    out, k = [], 0
    for name in GOLDEN_FILES:
        w, h = golden_size(name)
        W, H = GOLDEN_SIZES[name]
        for f in bc.FILTERS:
            for b in GOLDEN_BOXES:
                box, mirror = bc.boxes(w, h)[b], bool(k & 1)
                k += 1
                out.append(("%s>%dx%d %s %s m%d" % (name, W, H, f, b, mirror), name, W, H, f, box, mirror))
    return out


def golden_size(name):
    """width, height from the file's SOF0 (no decoder needed)"""
    data = open(os.path.join(HERE, name), "rb").read()
    at = data.index(b"\xff\xc0")
    return int.from_bytes(data[at + 7:at + 9], "big"), int.from_bytes(data[at + 5:at + 7], "big")


def pins():
    import PIL
    from PIL import Image
    srcs = bc.sources()
    out = {"resizer": "Pillow %s: Image.resize((W, H), filter, box=box) on 8-bit images (modes RGB and L), then FLIP_LEFT_RIGHT "
                      "where mirror=1; libjpeg_sha256: the same of Image.open(f).convert('RGB')" % PIL.__version__,
           "sha256": {}, "libjpeg_sha256": {}, "span_sha256": {}}
    # one axis on which the span taken in single and in double precision give different taps (tests/test_resize_box_reference.py)
    out["span_sha256"]["span51"] = bc.sha256(pillow_resize_box(bc.rc.noise(51, 1, 0), 14, 1, "bicubic",
                                                               (4.75789737701416, 0.0, 24.519044876098633, 1.0), False))
    for pin, name, W, H, f, box, mirror in bc.cases(srcs):
        out["sha256"][pin] = bc.sha256(pillow_resize_box(srcs[name], W, H, f, box, mirror))
    for pin, name, W, H, f, box, mirror in golden_cases():
        img = Image.open(io.BytesIO(open(os.path.join(HERE, name), "rb").read())).convert("RGB")
        out["libjpeg_sha256"][pin] = bc.sha256(pillow_resize_box(img, W, H, f, box, mirror))
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "resize_box_pins.json"), "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
