"""tools/resize_reference.py -- the numpy definition of the resizing step (include/hvc_jpeg.h, Resizing) -- held to Pillow's
Image.resize with 0 mismatching bytes where Pillow imports, and everywhere to the pins of tests/golden/resize_pins.json
(SHA-256 of Pillow's output, made by tests/golden/make_resize_pins.py).  No GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest

import resize_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import resize_reference as rr  # noqa: E402


def pil():
    return pytest.importorskip("PIL.Image")


def pillow_resize(img, W, H, f):
    Image = pil()
    return np.asarray(Image.fromarray(img).resize((W, H), {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[f]))


def mismatches(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, (a.shape, b.shape)
    return int(np.count_nonzero(a != b))


@pytest.fixture(scope="module")
def srcs():
    return rc.sources()


def test_reference_stands_alone():
    text = open(os.path.join(ROOT, "tools", "resize_reference.py")).read()
    assert re.findall(r"^\s*(?:import|from)\s+(\S+)", text, flags=re.M) == ["numpy"]


# ---- against Pillow itself
@pytest.mark.parametrize("w,h", rc.IN_SIZES)
def test_noise_images_equal_pillow(w, h):
    """1 x 1 up to 480 x 320 to 1 x 1, 2 x 2, 8 x 8, 31 x 17, 224 x 224, the same size, one axis the same, 2x and 3x: all filters"""
    img = rc.noise(w, h)
    for W, H in rc.out_sizes(w, h):
        for f in rc.FILTERS:
            assert mismatches(rr.resize(img, W, H, f), pillow_resize(img, W, H, f)) == 0, (W, H, f)


def test_one_channel_and_planar_equal_pillow():
    img = rc.noise(53, 45, 3)
    for W, H in ((24, 16), (53, 16), (106, 90), (7, 45)):
        for f in rc.FILTERS:
            want = np.stack([pillow_resize(np.ascontiguousarray(img[:, :, c]), W, H, f) for c in range(3)])
            assert mismatches(rr.resize_planar(np.ascontiguousarray(img.transpose(2, 0, 1)), W, H, f), want) == 0
            assert mismatches(rr.resize(np.ascontiguousarray(img[:, :, 1]), W, H, f), want[1]) == 0
            # a plane of its own is a channel of the interleaved image: the passes do not mix channels
            assert mismatches(rr.resize(img, W, H, f), np.ascontiguousarray(want.transpose(1, 2, 0))) == 0


@pytest.mark.parametrize("name", rc.GOLDEN_FILES)
def test_decoded_golden_files_equal_pillow(name, srcs):
    img = srcs[name]
    h, w = img.shape[:2]
    for W, H in ((224, 224), (31, 17), (w // 2, h // 2), (w, 100), (1, 1)):
        for f in rc.FILTERS:
            assert mismatches(rr.resize(img, W, H, f), pillow_resize(img, W, H, f)) == 0, (W, H, f)


def test_constant_images_and_the_checkerboard_equal_pillow():
    for v in (0, 255):
        img = np.full((9, 17, 3), v, dtype=np.uint8)
        for W, H in rc.out_sizes(17, 9):
            for f in rc.FILTERS:
                got = rr.resize(img, W, H, f)
                assert mismatches(got, pillow_resize(img, W, H, f)) == 0
                assert (got == v).all()                      # the taps of a position sum to 2^22 closely enough: a constant stays
    img = rc.checkerboard(53, 45)
    for W, H in rc.out_sizes(53, 45):
        got = rr.resize(img, W, H, "bicubic")
        assert mismatches(got, pillow_resize(img, W, H, "bicubic")) == 0


def test_the_checkerboard_takes_both_sides_of_the_clip():
    """under bicubic 2x the sums before the clip leave 0 .. 255 on both sides"""
    img = rc.checkerboard(53, 45)
    xmin, count, taps = rr.coefficients(53, 106, "bicubic")
    row = img[0, :, 0].astype(np.int64)
    sums = np.array([(taps[p, :count[p]] * row[xmin[p]:xmin[p] + count[p]]).sum() + (1 << 21) for p in range(106)]) >> 22
    assert sums.min() < 0 and sums.max() > 255
    out = rr.resize(img, 106, 90, "bicubic")
    assert out.min() == 0 and out.max() == 255


def test_refusals():
    img = rc.noise(5, 7)
    for bad in (lambda: rr.resize(img, 0, 4), lambda: rr.resize(img, 4, -1), lambda: rr.resize(img, 4, 4, "lanczos"),
                lambda: rr.coefficients(0, 4, "box"), lambda: rr.resize(img.astype(np.int16), 4, 4)):
        with pytest.raises(ValueError):
            bad()


def test_the_accumulator_fits_int32():
    """255 * SUM |k| + 2^21 < 2^31 over a sweep of its own; the largest sum found is bicubic 69 -> 64"""
    worst = (0, None)
    for n_in in list(range(1, 130)) + [255, 256, 257, 480, 1080, 1920]:
        for n_out in (1, 2, 3, 7, 8, 31, 64, 100, 224, 256, 1000):
            for f in rc.FILTERS:
                worst = max(worst, (rr.max_abs_tap_sum(n_in, n_out, f), (n_in, n_out, f)))
    assert worst == (5321270, (69, 64, "bicubic")) and 255 * worst[0] + (1 << 21) < (1 << 31)


# ---- the pins
def stored_pins():
    with open(os.path.join(ROOT, "tests", "golden", "resize_pins.json")) as f:
        return json.load(f)["sha256"]


def test_pins_are_what_pillow_resizes_today():
    pil()
    import make_resize_pins
    assert make_resize_pins.pins()["sha256"] == stored_pins()


def test_reference_reproduces_the_pins(srcs):
    """without Pillow: the definition against the stored hashes"""
    stored = stored_pins()
    cases = rc.cases(srcs)
    assert len(stored) == len(cases) and len(cases) > 300
    for pin, name, W, H, f in cases:
        assert rc.sha256(rr.resize(srcs[name], W, H, f)) == stored[pin], pin


def test_header_states_the_definition():
    header = open(os.path.join(ROOT, "include", "hvc_jpeg.h")).read()
    assert re.search(r"typedef enum \{ HVC_RESIZE_BOX = 0, HVC_RESIZE_BILINEAR = 1, HVC_RESIZE_BICUBIC = 2 \} hvc_resize_filter;", header)
    assert "#define HVC_RESIZE_MAX_TAPS 2048" in header and "Resizing" in header
    from video_coding_amd import hvc
    assert hvc.HVC_RESIZE == {"box": 0, "bilinear": 1, "bicubic": 2} and hvc.HVC_RESIZE_MAX_TAPS == 2048
