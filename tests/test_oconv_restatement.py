"""A second restatement of `oyuv convert`'s plane operations, written from the OCaml text in whole-array numpy slicing, against
the first one (oracle/hvc_oracle.c, loops over samples).  The oracle is what every GPU test of csrc/hvc_yuv.hip compares with,
and the reference's own expect tests pin it only at 4 x 4, where no row has an interior column beside the last one and no
crop clamps; a misreading of the OCaml shared by the oracle and the kernels would pass there.  Two restatements that share no
structure agreeing byte for byte at every small size, odd sizes and clamped crops included, is the check there is without
the OCaml tool chain.  Where they disagree, the OCaml text decides."""
import itertools

import numpy as np
import pytest

from conftest import golden_json
from oracle import orc

WIDTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33)
HEIGHTS = (1, 2, 3, 5)
FORMATS = [420, 422, 444, "YUY2", "UYVY", "YVYU"]
PACKED_OFFSETS = {"YUY2": (0, 1, 3), "UYVY": (1, 0, 2), "YVYU": (0, 3, 1)}      # tools/src/packed_422.ml:6-8


# ---- the restatement --------------------------------------------------------------------------------------------------------
def avg2(a, b):
    """tools/src/planar_444.ml:4-8"""
    return ((a.astype(np.int64) + b + 1) >> 1).astype(np.uint8)


def avg4(a, b, c, d):
    """tools/src/planar_444.ml:10-16"""
    return ((a.astype(np.int64) + b + c + d + 2) >> 2).astype(np.uint8)


def right_of(p):
    """every sample's right neighbour; the last column's is itself (what :31-32 and :97-102 write, as avg2 a a = a)"""
    w = p.shape[1]
    return p[:, np.minimum(np.arange(w) + 1, w - 1)]


def below(p):
    """tools/src/planar_444.ml:86: row2 = min (h - 1) (row + 1)"""
    h = p.shape[0]
    return p[np.minimum(np.arange(h) + 1, h - 1), :]


def subsample_h2(src, dw, dh):
    """tools/src/planar_444.ml:18-23 for every row of a dw x dh destination"""
    return avg2(src[:dh, 0:2 * dw:2], src[:dh, 1:2 * dw:2])


def subsample_hv2(src, dw, dh):
    """tools/src/planar_444.ml:69-80 for every row of a dw x dh destination"""
    even, odd = src[0:2 * dh:2], src[1:2 * dh:2]
    return avg4(even[:, 0:2 * dw:2], even[:, 1:2 * dw:2], odd[:, 0:2 * dw:2], odd[:, 1:2 * dw:2])


def supersample_h2(src):
    """tools/src/planar_444.ml:25-33 for every row"""
    h, w = src.shape
    dst = np.empty((h, 2 * w), np.uint8)
    dst[:, 0::2] = src
    dst[:, 1::2] = avg2(src, right_of(src))
    return dst


def supersample_hv2(src):
    """tools/src/planar_444.ml:82-103 for every row"""
    h, w = src.shape
    a, c = src, below(src)
    b, d = right_of(a), right_of(c)
    dst = np.empty((2 * h, 2 * w), np.uint8)
    dst[0::2, 0::2] = a
    dst[0::2, 1::2] = avg2(a, b)
    dst[1::2, 0::2] = avg2(a, c)
    dst[1::2, 1::2] = avg4(a, b, c, d)      # (last column: avg4 a a c c = avg2 a c, :101-102)
    return dst


def crop(src, dw, dh, x_pos, y_pos):
    """tools/src/yuv.ml:43-62 of one plane"""
    h, w = src.shape
    cols = np.clip(np.arange(dw) + x_pos, 0, w - 1)
    rows = np.clip(np.arange(dh) + y_pos, 0, h - 1)
    return src[rows][:, cols]


def packed_to_planar(fmt, src, w, h):
    """tools/src/packed_422.ml:10-23: a (2 w) x h plane -> the planes of a 4:2:2 frame of luma size w x h (w even)"""
    yo, uo, vo = PACKED_OFFSETS[fmt]
    quads = src.reshape(h, w // 2, 4)
    y = np.empty((h, w), np.uint8)
    y[:, 0::2], y[:, 1::2] = quads[:, :, yo], quads[:, :, yo + 2]
    return y, quads[:, :, uo].copy(), quads[:, :, vo].copy()


def packed_from_planar(fmt, y, u, v):
    """tools/src/packed_422.ml:33-46"""
    yo, uo, vo = PACKED_OFFSETS[fmt]
    h, w = y.shape
    quads = np.empty((h, w // 2, 4), np.uint8)
    quads[:, :, yo], quads[:, :, yo + 2], quads[:, :, uo], quads[:, :, vo] = y[:, 0::2], y[:, 1::2], u, v
    return quads.reshape(h, 2 * w)


def planes_of(raw, w, h, cw, ch):
    return raw[:w * h].reshape(h, w), raw[w * h:w * h + cw * ch].reshape(ch, cw), raw[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)


def oconv(raw, fmt_in, size_in, fmt_out, size_out, offset=(0, 0)):
    """One pass of the loop of tools/src/oconv.ml:111-133: input (:12-25) into a 4:4:4 frame, Yuv.crop, output (:35-47)"""
    (w, h), (w2, h2) = size_in, size_out
    if fmt_in in PACKED_OFFSETS:
        y, u, v = packed_to_planar(fmt_in, raw[:2 * w * h], w, h)
        u, v = supersample_h2(u), supersample_h2(v)
    elif fmt_in == 420:
        y, u, v = planes_of(raw, w, h, w // 2, h // 2)
        u, v = supersample_hv2(u), supersample_hv2(v)
    elif fmt_in == 422:
        y, u, v = planes_of(raw, w, h, w // 2, h)
        u, v = supersample_h2(u), supersample_h2(v)
    else:
        y, u, v = planes_of(raw, w, h, w, h)
    y, u, v = (crop(p, w2, h2, *offset) for p in (y, u, v))
    if fmt_out == 420:
        u, v = subsample_hv2(u, w2 // 2, h2 // 2), subsample_hv2(v, w2 // 2, h2 // 2)
    elif fmt_out != 444:
        u, v = subsample_h2(u, w2 // 2, h2), subsample_h2(v, w2 // 2, h2)
    if fmt_out in PACKED_OFFSETS:
        return packed_from_planar(fmt_out, y, u, v).tobytes()
    return y.tobytes() + u.tobytes() + v.tobytes()


def frame_bytes(fmt, w, h):
    return {420: w * h + 2 * (w // 2) * (h // 2), 444: 3 * w * h}.get(fmt, 2 * w * h)


# ---- restatement against oracle ------------------------------------------------------------------------------------------------
def planes():
    rng = np.random.Generator(np.random.PCG64(1906))
    for w, h in itertools.product(WIDTHS, HEIGHTS):
        yield rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        yield np.where(rng.integers(0, 2, size=(h, w)) == 1, 255, 254).astype(np.uint8)       # (no sum may wrap in 8 bits)


def test_sub_and_supersampling_agree_with_the_oracle():
    """tools/src/planar_444.ml:18-33, 69-103 at every width x height, odd sizes (the last source column / row unused) included"""
    for p in planes():
        h, w = p.shape
        assert np.array_equal(supersample_h2(p), orc.supersample_h2(p)), (w, h)
        assert np.array_equal(supersample_hv2(p), orc.supersample_hv2(p)), (w, h)
        assert np.array_equal(subsample_h2(p, w // 2, h), orc.subsample_h2(p, w // 2, h)), (w, h)
        assert np.array_equal(subsample_hv2(p, w // 2, h // 2), orc.subsample_hv2(p, w // 2, h // 2)), (w, h)


def test_crop_agrees_with_the_oracle():
    """tools/src/yuv.ml:43-62: the window inside, shifted out of each of the four edges (partly and wholly), out of two at
    once, larger than the source on every side"""
    for p in planes():
        h, w = p.shape
        windows = [(w, h, 0, 0), (max(1, w - 1), max(1, h - 1), 1 if w > 1 else 0, 1 if h > 1 else 0),
                   (w, h, -2, 0), (w, h, 2, 0), (w, h, 0, -2), (w, h, 0, 2),                  # out of one edge
                   (3, 2, -5, 0), (3, 2, w + 1, 0), (3, 2, 0, -4), (3, 2, 0, h + 1),          # wholly outside it
                   (w, h, -1, 1), (w, h, 1, -1),
                   (w + 5, h + 4, -3, -2), (w + 9, h + 1, 0, 0), (2 * w + 1, 3 * h, -w, -h)]  # larger than the source
        for dw, dh, x, y in windows:
            assert np.array_equal(crop(p, dw, dh, x, y), orc.crop_plane(p, dw, dh, x, y)), (w, h, dw, dh, x, y)


def test_packed_422_agrees_with_the_oracle():
    """tools/src/packed_422.ml:6-44, every byte order; the chroma width runs over the width list (the luma width is twice it)"""
    rng = np.random.Generator(np.random.PCG64(422))
    for cw, h, fmt in itertools.product(WIDTHS, HEIGHTS, PACKED_OFFSETS):
        w = 2 * cw
        src = rng.integers(0, 256, size=(h, 2 * w), dtype=np.uint8)
        mine, theirs = packed_to_planar(fmt, src, w, h), orc.packed422_to_planar(orc.PACKED[fmt], src, w, h)
        for a, b in zip(mine, theirs):
            assert np.array_equal(a, b), (fmt, w, h)
        assert np.array_equal(packed_from_planar(fmt, *mine), src), (fmt, w, h)                # every byte has one place
        y, u, v = (rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((h, w), (h, cw), (h, cw)))
        assert np.array_equal(packed_from_planar(fmt, y, u, v), orc.packed422_from_planar(orc.PACKED[fmt], y, u, v)), (fmt, w, h)


OCONV_CASES = ([(s, s, (0, 0)) for s in ((2, 2), (6, 2), (18, 6), (70, 34))] +
               [((18, 6), (10, 4), (3, 1)), ((18, 6), (26, 10), (-5, -2)), ((70, 34), (32, 16), (9, 5)), ((70, 34), (34, 40), (-6, -4))])


@pytest.mark.parametrize("fmt_in", FORMATS)
@pytest.mark.parametrize("fmt_out", FORMATS)
def test_oconv_agrees_with_the_oracle(fmt_in, fmt_out):
    """tools/src/oconv.ml:12-47, 111-133: every format pair, same size and cropped at an inside and at a negative offset"""
    rng = np.random.Generator(np.random.PCG64(FORMATS.index(fmt_in) * 6 + FORMATS.index(fmt_out)))
    for size_in, size_out, off in OCONV_CASES:
        raw = rng.integers(0, 256, size=frame_bytes(fmt_in, *size_in), dtype=np.uint8)
        mine = oconv(raw, fmt_in, size_in, fmt_out, size_out, off)
        assert len(mine) == frame_bytes(fmt_out, *size_out)
        assert mine == orc.oconv_frame(raw, fmt_in, size_in, fmt_out, size_out, off), (fmt_in, fmt_out, size_in, size_out, off)


# ---- restatement against the reference's own expect tests ---------------------------------------------------------------------
A = lambda rows: np.array(rows, dtype=np.uint8)


def test_g7_upsample_frames_through_the_restatement():
    """tools/src/planar_444.ml:139-249"""
    g = golden_json("g7_upsample.json")["cases"]
    f444, f420, back = g["444<->420"]
    for lo, hi, c0, c1 in ((4, 8, 4, 6), (8, 12, 6, 8)):
        assert subsample_hv2(A(f444[lo:hi]), 2, 2).tolist() == f420[c0:c1]
        assert supersample_hv2(A(f420[c0:c1])).tolist() == back[lo:hi]
    f444, f422, back = g["444<->422"]
    for lo, hi in ((4, 8), (8, 12)):
        assert subsample_h2(A(f444[lo:hi]), 2, 4).tolist() == f422[lo:hi]
        assert supersample_h2(A(f422[lo:hi])).tolist() == back[lo:hi]
    flat = lambda rows: np.concatenate([A(r) for r in rows])
    assert oconv(flat(g["444<->420"][0]), 444, (4, 4), 420, (4, 4)) == flat(g["444<->420"][1]).tobytes()
    assert oconv(flat(g["444<->420"][1]), 420, (4, 4), 444, (4, 4)) == flat(g["444<->420"][2]).tobytes()
    assert oconv(flat(g["444<->422"][0]), 444, (4, 4), 422, (4, 4)) == flat(g["444<->422"][1]).tobytes()
    assert oconv(flat(g["444<->422"][1]), 422, (4, 4), 444, (4, 4)) == flat(g["444<->422"][2]).tobytes()


def test_g7_packed_frame_through_the_restatement():
    """tools/src/packed_422.ml:56-104"""
    g = golden_json("g7_packed422.json")
    assert g["format"] == "yuy2"
    y, u, v = A(g["frame"][0:4]), A(g["frame"][4:8]), A(g["frame"][8:12])
    packed = packed_from_planar("YUY2", y, u, v)
    assert packed.tolist() == g["packed"]
    y2, u2, v2 = packed_to_planar("YUY2", A(g["packed"]), 4, 4)
    assert y2.tolist() + u2.tolist() + v2.tolist() == g["unpacked"]
