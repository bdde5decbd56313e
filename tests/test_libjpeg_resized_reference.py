"""The reference chain of hvc_jpeg_decode_batch_mixed_resized under hvc_set_mixed_arithmetic(HVC_ARITH_LIBJPEG), on the CPU:
tools/resize_reference.py's resize of the libjpeg-exact image (tools/libjpeg_reference.py) against the pins of
tests/golden/libjpeg_resized_pins.json -- the SHA-256 of Pillow's Image.open(f).convert("RGB").resize((W, H), filter) -- and,
where Pillow imports, against Pillow itself.  Files: libjpeg_files.GOLDEN_FILES and PINNED; sizes (8, 8), (24, 16), (7, 5),
(32, 32); the three filters: 108 cases.  It is the yardstick tests/test_gpu_mixed_libjpeg.py holds the GPU against."""
import json
import os
import sys

import numpy as np
import pytest

import libjpeg_files as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import libjpeg_reference as lj  # noqa: E402
import make_libjpeg_resized_pins as mk  # noqa: E402
import resize_reference as rr  # noqa: E402


@pytest.fixture(scope="module")
def stored():
    with open(os.path.join(ROOT, "tests", "golden", "libjpeg_resized_pins.json")) as f:
        return json.load(f)["rgb_sha256"]


@pytest.fixture(scope="module")
def images():
    """name -> (bytes, the libjpeg-exact RGB image by the definition): decoded once"""
    from video_coding_amd import hvc
    out = {}
    for name, data in mk.files().items():
        info, coefs = hvc.jpeg_entropy_decode(data, restart_markers=True)
        out[name] = (data, lj.record_to_rgb(coefs, info.qtab_array(), lf.planes_of_info(info), lf.sampling_of_info(info), info.width, info.height))
    return out


def test_the_cases_are_the_108():
    assert mk.SIZES == [(8, 8), (24, 16), (7, 5), (32, 32)] and mk.FILTERS == ["box", "bilinear", "bicubic"]
    assert list(mk.files()) == lf.GOLDEN_FILES + [lf.pin_name(*c) for c in lf.PINNED]
    assert len(mk.files()) * len(mk.SIZES) * len(mk.FILTERS) == 108


def test_reference_chain_reproduces_the_pins(stored, images):
    assert len(stored) == 108
    bad = []
    for name, (_, rgb) in images.items():
        for w, h in mk.SIZES:
            for filt in mk.FILTERS:
                if lf.sha256(rr.resize(rgb, w, h, filt)) != stored[mk.pin_key(name, w, h, filt)]:
                    bad.append(mk.pin_key(name, w, h, filt))
    assert bad == []


def test_pins_are_what_pillow_gives_today(stored):
    pytest.importorskip("PIL.Image")
    assert mk.pins()["rgb_sha256"] == stored


def test_reference_chain_equals_pillow(images):
    pytest.importorskip("PIL.Image")
    bad = n = 0
    for name, (data, rgb) in images.items():
        for w, h in mk.SIZES:
            for filt in mk.FILTERS:
                want = mk.pillow_resized(data, w, h, filt)
                got = rr.resize(rgb, w, h, filt)
                assert got.shape == want.shape == (h, w, 3)
                bad += int(np.count_nonzero(got != want))
                n += 1
    assert n == 108 and bad == 0
