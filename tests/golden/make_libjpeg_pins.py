"""Writes tests/golden/libjpeg_pins.json: the SHA-256 of the RGB image libjpeg-turbo (through Pillow) decodes from the two
golden files and from a handful of files written by tools/jpeg_opt_writer.py (tests/libjpeg_files.py PINNED: each is named
by its size, sampling, coefficient family and seed).  tests/test_libjpeg_reference.py regenerates and compares them where
Pillow is installed; tests/test_gpu_libjpeg.py holds the GPU's bytes against them where it is not.

    python tests/golden/make_libjpeg_pins.py"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import libjpeg_files as lf  # noqa: E402


def pillow_rgb(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))   # (a one-component file decodes to "L": R = G = B = Y)


def pins():
    import PIL
    out = {"decoder": "Pillow %s (bundled libjpeg-turbo), default settings" % PIL.__version__, "rgb_sha256": {}}
    for name in lf.GOLDEN_FILES:
        with open(os.path.join(HERE, name), "rb") as f:
            out["rgb_sha256"][name] = lf.sha256(pillow_rgb(f.read()))
    for case in lf.PINNED:
        out["rgb_sha256"][lf.pin_name(*case)] = lf.sha256(pillow_rgb(lf.pinned_file(case)[0]))
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "libjpeg_pins.json"), "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
