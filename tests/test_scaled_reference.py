"""tools/scaled_reference.py -- the numpy statement of the reduced-size inverse DCT (include/hvc_jpeg.h, "Decoding at
reduced size") -- against libjpeg-turbo's scale_denom through PIL, and hvc_jpeg_scaled_info's sizes against PIL's.
CPU only: the files come from tools/jpeg_opt_writer.py, written from random coefficient records."""
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scaled_reference as sr  # noqa: E402
from jpeg_opt_writer import jpeg_optimised_tables  # noqa: E402

Image = pytest.importorskip("PIL.Image")
from PIL import ImageFile  # noqa: E402


def pil_scaled(data, mode, s):
    """the file decoded by libjpeg with scale_denom = s.  Image.draft() does it where it can: it derives the scale from a
    requested size, min(w // size[0], h // size[1]) rounded down to 8, 4, 2, 1.  It cannot reach 1/8 for an image narrower
    than 8 (nor any scale for a width of 1), so for those the fields draft() sets are set here directly -- PIL internals
    (im._mode, im._size, im.tile, im.decoderconfig as JpegImageFile.draft of Pillow 9 ... 12 leaves them; written against
    Pillow 12.2): if a later Pillow changes them, this branch is what breaks, not the definition under test."""
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    if min(w, h) // s >= 1 and min(w // (w // s), h // (h // s)) < 2 * s:
        im.draft(mode, (w // s, h // s))
    else:
        d, e, o, a = im.tile[0]
        if a[0] == "RGB" and mode in ("L", "YCbCr"):
            im._mode = mode
            a = mode, ""
        im._size = ((w + s - 1) // s, (h + s - 1) // s)
        im.tile = [ImageFile._Tile(d, (e[0], e[1], e[0] + im._size[0], e[1] + im._size[1]), o, a)]
        im.decoderconfig = (s, 0)
    assert im.decoderconfig[0] == s and im.size == ((w + s - 1) // s, (h + s - 1) // s)
    im.load()
    return im


def random_record(seed, w, h, n_comp, density, cmax, qmax):
    """(qtabs [2][64], coefs [n_comp][bh][bw][64]) with |DC * q| <= 1000: inside libjpeg's unmasked range"""
    rng = np.random.default_rng(seed)
    bw, bh = (w + 7) // 8, (h + 7) // 8
    q = rng.integers(1, qmax + 1, size=(2, 64)).astype(np.uint16)
    c = rng.integers(-cmax, cmax + 1, size=(n_comp, bh, bw, 64))
    c *= rng.random(size=c.shape) < density
    for k in range(n_comp):
        lim = 1000 // int(q[min(k, 1), 0])
        c[k, ..., 0] = rng.integers(-lim, lim + 1, size=(bh, bw))
    return q, c.astype(np.int16)


FILES = [  # (w, h, density, |c| <=, q <=)
    (32, 24, 0.15, 60, 12),
    (64, 40, 0.50, 25, 30),
    (16, 16, 1.00, 8, 255),
    (40, 32, 0.05, 1023, 3),
]


@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("case", range(len(FILES)))
def test_reference_equals_libjpeg_444(case, s):
    w, h, density, cmax, qmax = FILES[case]
    q, c = random_record(100 + case, w, h, 3, density, cmax, qmax)
    data = jpeg_optimised_tables(w, h, 444, q, c)
    got = np.asarray(pil_scaled(data, "YCbCr", s))
    n = 8 // s
    sw, sh = sr.scaled_size(w, n), sr.scaled_size(h, n)
    assert got.shape == (sh, sw, 3)
    bad = 0
    for k in range(3):
        want = sr.scaled_plane(c[k], q[min(k, 1)], c.shape[2], c.shape[1], n)[:sh, :sw]
        bad += int(np.count_nonzero(want != got[:, :, k]))
    assert bad == 0


@pytest.mark.parametrize("s", [2, 4, 8])
def test_reference_equals_libjpeg_one_component(s):
    w, h = 24, 40
    q, c = random_record(7, w, h, 1, 0.3, 40, 20)
    data = jpeg_optimised_tables(w, h, [(1, 1)], q, c)
    got = np.asarray(pil_scaled(data, "L", s))
    n = 8 // s
    want = sr.scaled_plane(c[0], q[0], c.shape[2], c.shape[1], n)[:sr.scaled_size(h, n), :sr.scaled_size(w, n)]
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("w", [1, 7, 8, 9, 17])
def test_scaled_info_sizes_equal_pils(w):
    from video_coding_amd import hvc
    h = 17
    q, c = random_record(3, w, h, 3, 0.1, 10, 10)
    data = jpeg_optimised_tables(w, h, 444, q, c)
    info = hvc.jpeg_read_header(data)
    for s in (1, 2, 4, 8):
        n = 8 // s
        si = hvc.jpeg_scaled_info(info, s)
        assert (si.width, si.height) == pil_scaled(data, "YCbCr", s).size
        at = 0
        for k in range(3):
            assert (si.comp[k].actual_width, si.comp[k].actual_height) == (si.width, si.height)
            assert (si.comp[k].decoded_width, si.comp[k].decoded_height) == (info.comp[k].decoded_width * n // 8, info.comp[k].decoded_height * n // 8)
            L, L0 = si.layout[k], info.layout[k]
            assert (L.blocks_w, L.blocks_h, L.qtab, L.coef_offset) == (L0.blocks_w, L0.blocks_h, L0.qtab, L0.coef_offset)
            assert (L.stride, L.plane_offset) == (L.blocks_w * n, at)
            at += L.blocks_w * n * L.blocks_h * n
        assert si.pixel_bytes == at and si.coef_count == info.coef_count
        assert np.array_equal(si.qtab_array(), info.qtab_array())
    with pytest.raises(hvc.HvcError) as e:
        hvc.jpeg_scaled_info(info, 3)
    assert e.value.code == -1
