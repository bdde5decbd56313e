"""The numpy definition of the libjpeg-exact encoder (tools/libjpeg_encode_reference.py; include/hvc_jpeg.h "Encoding
bit-exact to libjpeg") against libjpeg-turbo itself: Pillow writes a file with our tables, this library's host reader gives
the file's coefficient records, and the definition's record must equal them whole -- 0 mismatching coefficients, dummy
blocks included.  Where Pillow does not import, the pins of tests/golden/libjpeg_encode_pins.json (SHA-256 of Pillow's
records, made by tests/golden/make_libjpeg_encode_pins.py) hold the definition instead; they are checked everywhere."""
import json

import numpy as np
import pytest

import libjpeg_encode_cases as lc

CASES = lc.plane_cases() + lc.rgb_cases()
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def references():
    """every case's record, computed once"""
    return {c[0]: lc.reference_record(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_definition_equals_pillow(case, references):
    pytest.importorskip("PIL.Image")
    info, got = lc.file_record(lc.pillow_file(case), case[5])
    want = references[case[0]]
    geo = lc.ler.geometry(case[1], case[2], case[3])
    assert [(info.layout[k].blocks_w, info.layout[k].blocks_h) for k in range(info.n_comp)] == [(g[0], g[1]) for g in geo]
    assert got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d coefficients differ, first in block %d at zig-zag position %d" % (bad.size, bad[0] // 64, bad[0] % 64)


def test_definition_equals_pins(references):
    with open(lc.PINS) as f:
        pins = json.load(f)
    assert sorted(pins) == sorted(IDS), "the pins are not the cases: run tests/golden/make_libjpeg_encode_pins.py"
    wrong = [name for name in IDS if lc.sha256(references[name].astype("<i2")) != pins[name]]
    assert not wrong, wrong


def test_dummy_rule_cases_have_dummies():
    """the grid does cross the rules it is there for"""
    def dummies(w, h, s):
        bw, bh, hs, vs = lc.ler.geometry(w, h, s)[0]
        return bw - -(-w // 8), bh - -(-h // 8)
    assert dummies(40, 24, 420) == (1, 1) and dummies(16, 24, 420) == (0, 1) and dummies(24, 24, 420) == (1, 1)
    assert dummies(24, 16, 420) == (1, 0) and dummies(24, 16, 422) == (1, 0) and dummies(17, 9, 444) == (0, 0)
    # the corner of 24 x 24 chains through the dummy to its left... of the row above
    assert lc.ler.dummy_source(3, 3, 3, 3, 2, 2) == (2, 2) and lc.ler.dummy_source(2, 3, 3, 3, 2, 2) == (2, 2)
    assert lc.ler.dummy_source(0, 3, 3, 3, 2, 2) == (1, 2) and lc.ler.dummy_source(3, 0, 3, 3, 2, 2) == (2, 0)


def test_the_models_422_factors_add_only_dummy_rows(references):
    """This library's 4:2:2 files are 2x2 / 1x2 / 1x2 (the model's Parameters.c422), Pillow's 2x1 / 1x1 / 1x1.  Where the
    height is whole 16-row MCUs the records are the same; elsewhere the model's layout has one block row more per plane,
    all dummies, and the rows above it are Pillow's."""
    model = [(2, 2), (1, 2), (1, 2)]
    for case in CASES:
        name, w, h, s, kind, tab = case
        if s != 422 or name.startswith("rgb_"):
            continue
        planes = lc.component_planes(w, h, s, kind)
        got = lc.ler.encode_planes(planes, w, h, s, lc.tables(tab), factors=model)
        at_m, at_p = 0, 0
        for plane, (bw, bh, hs, _), (pw, ph, _, _) in zip(planes, lc.ler.geometry(w, h, s, model), lc.ler.geometry(w, h, s)):
            m = got[at_m:at_m + bw * bh * 64].reshape(bh, bw, 64)
            p = references[name][at_p:at_p + pw * ph * 64].reshape(ph, pw, 64)
            assert bw == pw and bh in (ph, ph + 1) and np.array_equal(m[:ph], p)
            if bh > ph:   # the dummy row: AC 0, the DC of the MCU's last block of the row above (or of the last real one)
                real_w = -(-plane.shape[1] // 8)
                assert not m[ph, :, 1:].any()
                assert all(m[ph, bx, 0] == m[ph - 1, min(bx // hs * hs + hs - 1, real_w - 1), 0] for bx in range(bw))
            at_m, at_p = at_m + bw * bh * 64, at_p + pw * ph * 64


def test_bias_alternates():
    a = np.full((2, 8), 1, dtype=np.uint8)
    a[1, :] = 2  # sums 6: (6 + 1) >> 2 = 1, (6 + 2) >> 2 = 2
    assert lc.ler.downsample_h2v2(a).tolist() == [[1, 2, 1, 2]]
    b = np.array([[1, 2] * 4], dtype=np.uint8)  # sums 3: (3 + 0) >> 1 = 1, (3 + 1) >> 1 = 2
    assert lc.ler.downsample_h2v1(b).tolist() == [[1, 2, 1, 2]]
