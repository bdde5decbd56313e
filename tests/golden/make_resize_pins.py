"""Writes tests/golden/resize_pins.json: the SHA-256 of what Pillow's Image.resize makes of the images of tests/resize_cases.py
(seeded noise from 1 x 1 to 480 x 320, constant and checkerboard images, the two decoded golden files) at the output sizes and
under the three filters listed there.  tests/test_resize_reference.py regenerates and compares them where Pillow is
installed, and holds tools/resize_reference.py against them everywhere.

    python tests/golden/make_resize_pins.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_cases as rc  # noqa: E402


def pillow_resize(img, W, H, filter):
    from PIL import Image
    f = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filter]
    return np.asarray(Image.fromarray(img).resize((W, H), f))


def pins():
    import PIL
    srcs = rc.sources()
    out = {"resizer": "Pillow %s, Image.resize on 8-bit images (modes RGB and L), default settings" % PIL.__version__, "sha256": {}}
    for pin, name, W, H, f in rc.cases(srcs):
        out["sha256"][pin] = rc.sha256(pillow_resize(srcs[name], W, H, f))
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "resize_pins.json"), "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
