"""tools/resize_reference.py resize_box / coefficients_box / apply_lut -- the numpy definition of the box, the mirror and the
typed output (include/hvc_jpeg.h, Resizing) -- against Pillow itself where it imports, and everywhere against the stored
hashes of Pillow's output (tests/golden/resize_box_pins.json).  0 mismatching bytes; no GPU."""
import json
import os
import sys

import numpy as np
import pytest

import resize_box_cases as bc
import resize_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_resize_box_pins as mk  # noqa: E402
import resize_reference as rr  # noqa: E402


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(ROOT, "tests", "golden", "resize_box_pins.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def srcs():
    return bc.sources()


def test_the_cases_cover_what_they_claim(srcs):
    cases = bc.cases(srcs)
    assert len({c[0] for c in cases}) == len(cases) > 250
    assert {c[1] for c in cases} >= {"noise1x1", "noise53x45", "grey53x45"}                       # from 1 x 1; L and RGB
    assert {c[4] for c in cases} == set(bc.FILTERS)
    for kind in bc.boxes(17, 9):                                                                  # every kind of box, both mirror flags
        named = [c for c in cases if c[1] == "noise17x9" and c[5] == bc.boxes(17, 9)[kind]]
        assert {c[6] for c in named} == {False, True}, kind
    thin = bc.boxes(53, 45)["thin"]
    assert thin[2] - thin[0] < 1 and thin[3] - thin[1] < 1
    b = bc.boxes(53, 45)
    assert b["left"][0] == 0 and b["top"][1] == 0 and b["right"][2] == 53 and b["bottom"][3] == 45
    assert any(c[2] > srcs[c[1]].shape[1] for c in cases) and any(c[2] < srcs[c[1]].shape[1] for c in cases)   # up and down


def test_resize_box_equals_the_pins(srcs, pins):
    cases = bc.cases(srcs)
    assert set(pins["sha256"]) == {c[0] for c in cases}
    bad = [pin for pin, name, W, H, f, box, mirror in cases if rc.sha256(rr.resize_box(srcs[name], W, H, f, box, mirror)) != pins["sha256"][pin]]
    assert bad == []


def test_resize_box_equals_pillow_itself(srcs, pins):
    pytest.importorskip("PIL")
    mismatching = 0
    for pin, name, W, H, f, box, mirror in bc.cases(srcs):
        want = mk.pillow_resize_box(srcs[name], W, H, f, box, mirror)
        assert rc.sha256(want) == pins["sha256"][pin], pin                                       # the pins are this Pillow's
        mismatching += int(np.count_nonzero(rr.resize_box(srcs[name], W, H, f, box, mirror) != want))
    assert mismatching == 0


def test_the_golden_file_pins_are_pillows(pins):
    Image = pytest.importorskip("PIL.Image")
    import io
    cases = mk.golden_cases()
    assert set(pins["libjpeg_sha256"]) == {c[0] for c in cases}
    for pin, name, W, H, f, box, mirror in cases:
        with open(os.path.join(ROOT, "tests", "golden", name), "rb") as fh:
            img = Image.open(io.BytesIO(fh.read())).convert("RGB")
        assert (img.width, img.height) == mk.golden_size(name)
        assert rc.sha256(mk.pillow_resize_box(img, W, H, f, box, mirror)) == pins["libjpeg_sha256"][pin], pin


def test_without_a_box_and_a_mirror_it_is_resize(srcs):
    for name in ("noise1x1", "noise17x9", "noise53x45", "grey53x45"):
        img = srcs[name]
        h, w = img.shape[:2]
        for W, H in bc.out_sizes(w, h):
            for f in bc.FILTERS:
                want = rr.resize(img, W, H, f)
                assert np.array_equal(rr.resize_box(img, W, H, f), want)
                assert np.array_equal(rr.resize_box(img, W, H, f, box=(0, 0, w, h), mirror=False), want)
                assert np.array_equal(rr.resize_box(img, W, H, f, mirror=True), want[:, ::-1])
                for n_in, n_out in ((w, W), (h, H)):
                    for a, b in zip(rr.coefficients(n_in, n_out, f), rr.coefficients_box(n_in, n_out, f)):
                        assert np.array_equal(a, b)


def test_an_integer_box_is_not_crop_then_resize(srcs):
    """taps reach outside the box (never outside the image): Pillow's behaviour, and the definition's"""
    img = srcs["noise53x45"]
    box = (13, 11, 40, 30)
    got = rr.resize_box(img, 20, 14, "bicubic", box)
    assert not np.array_equal(got, rr.resize(img[11:30, 13:40], 20, 14, "bicubic"))
    xmin, count, _ = rr.coefficients_box(53, 20, "bicubic", 13, 40)
    assert xmin[0] < 13 and xmin[-1] + count[-1] > 40 and xmin.min() >= 0 and (xmin + count).max() <= 53


def test_the_span_is_subtracted_in_single_precision():
    """51 -> 14 under bicubic with the window [4.757897..., 24.519044...): the span in single and in double differ in their last
    bits, and so do three taps -- Pillow's are the single ones (the case is among the pins below)"""
    in0, in1 = SPAN_CASE[4], SPAN_CASE[5]
    assert float(np.float32(in1) - np.float32(in0)) != float(in1) - float(in0)
    xmin, count, taps = rr.coefficients_box(51, 14, "bicubic", in0, in1)
    # the same axis with the span taken in double: everything else as coefficients_box
    scale = (float(np.float32(in1)) - float(np.float32(in0))) / 14
    center = np.add(float(np.float32(in0)), np.multiply(np.add(np.arange(14, dtype=np.float64), 0.5), scale))
    x = np.multiply(np.add(np.subtract((np.arange(taps.shape[1])[None, :] + xmin[:, None]).astype(np.float64), center[:, None]), 0.5), 1.0 / scale)
    w = np.where(np.arange(taps.shape[1])[None, :] < count[:, None], rr._bicubic(x), 0.0)
    w = np.divide(w, np.cumsum(w, axis=1)[:, -1:])
    other = np.where(w < 0.0, np.trunc(np.subtract(np.multiply(w, 4194304.0), 0.5)), np.trunc(np.add(np.multiply(w, 4194304.0), 0.5))).astype(np.int64)
    assert np.abs(other - taps).max() > 0


SPAN_CASE = ("span51", 14, 1, "bicubic", 4.75789737701416, 24.519044876098633)   # (pin, W, H, filter, x0, x1) of a 51 x 1 grey row


def test_the_single_precision_case_equals_pillows(pins):
    pin, W, H, f, x0, x1 = SPAN_CASE
    img = rc.noise(51, 1, 0)
    assert rc.sha256(rr.resize_box(img, W, H, f, (x0, 0.0, x1, 1.0))) == pins["span_sha256"][pin]


def test_refusals():
    img = rc.noise(17, 9)
    for box in ((-0.5, 0, 17, 9), (0, -1, 17, 9), (0, 0, 17.5, 9), (0, 0, 17, 9.25), (5, 0, 5, 9), (6, 0, 5, 9), (0, 4, 17, 4),
                (float("nan"), 0, 17, 9), (0, 0, float("inf"), 9), (0, float("-inf"), 17, 9)):
        with pytest.raises(ValueError):
            rr.resize_box(img, 8, 8, "bilinear", box)
    assert rr.resize_box(img, 8, 8, "bilinear", (0, 0, 17, 9)).shape == (8, 8, 3)


def test_row_window():
    assert rr.row_window(45, 17, "bicubic") == (0, 45)
    lo, hi = rr.row_window(45, 17, "bilinear", 10.5, 20.25)
    xmin, count, _ = rr.coefficients_box(45, 17, "bilinear", 10.5, 20.25)
    assert (lo, hi) == (int(xmin[0]), int(xmin[-1] + count[-1])) and 0 < lo < hi < 45


def test_apply_lut():
    rng = np.random.default_rng(5)
    img = rc.noise(17, 9)
    for dt in (np.uint16, np.uint32, np.float32, np.float16):
        lut = rng.integers(0, 1 << 16, size=(3, 256)).astype(dt)
        got = rr.apply_lut(img, lut)
        assert got.dtype == lut.dtype and got.shape == img.shape
        for c in range(3):
            assert np.array_equal(np.ascontiguousarray(got[..., c]).view(np.uint8), lut[c][img[..., c]].view(np.uint8))
        planar = rr.apply_lut(np.ascontiguousarray(img.transpose(2, 0, 1)), lut, channel_axis=0)
        assert np.array_equal(planar.view(np.uint8), np.ascontiguousarray(got.transpose(2, 0, 1)).view(np.uint8))
    with pytest.raises(ValueError):
        rr.apply_lut(img, np.zeros((3, 255), np.uint16))
