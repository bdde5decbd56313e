"""Writes tests/golden/libjpeg_resized_pins.json: the SHA-256 of Pillow's Image.open(file).convert("RGB").resize((W, H), filter)
for the two golden files and the writer-made files of tests/libjpeg_files.py PINNED, at four sizes under the three filters:
what hvc_jpeg_decode_batch_mixed_resized gives under hvc_set_mixed_arithmetic(HVC_ARITH_LIBJPEG).
tests/test_libjpeg_resized_reference.py regenerates and compares them where Pillow is installed and holds the numpy chain
(tools/libjpeg_reference.py, tools/resize_reference.py) against them everywhere; tests/test_gpu_mixed_libjpeg.py holds the
GPU's bytes against them.

    python tests/golden/make_libjpeg_resized_pins.py"""
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import libjpeg_files as lf  # noqa: E402

SIZES = [(8, 8), (24, 16), (7, 5), (32, 32)]   # (W, H)
FILTERS = ["box", "bilinear", "bicubic"]


def files():
    """name -> bytes, in the order of the pins"""
    out = {}
    for name in lf.GOLDEN_FILES:
        with open(os.path.join(HERE, name), "rb") as f:
            out[name] = f.read()
    for case in lf.PINNED:
        out[lf.pin_name(*case)] = bytes(lf.pinned_file(case)[0])
    return out


def pin_key(name, w, h, filt):
    return "%s %dx%d %s" % (name, w, h, filt)


def pillow_resized(data, w, h, filt):
    from PIL import Image
    f = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filt]
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB").resize((w, h), f))


def pins():
    import PIL
    out = {"resizer": "Pillow %s (bundled libjpeg-turbo): Image.open(f).convert('RGB').resize((W, H), filter)" % PIL.__version__,
           "rgb_sha256": {}}
    for name, data in files().items():
        for w, h in SIZES:
            for filt in FILTERS:
                out["rgb_sha256"][pin_key(name, w, h, filt)] = lf.sha256(pillow_resized(data, w, h, filt))
    return out


if __name__ == "__main__":
    with open(os.path.join(HERE, "libjpeg_resized_pins.json"), "w") as f:
        json.dump(pins(), f, indent=1, sort_keys=True)
        f.write("\n")
