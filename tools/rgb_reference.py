"""The RGB image of a JPEG frame, and the planes of an RGB image, in numpy -- the definition csrc/hvc_rgb.hip is tested
against (include/hvc_jpeg.h, RGB).  Stands alone: numpy only, no import from the library or from the test oracle.

    full-size chroma   Planar_444.supersample_hv2 (4:2:0) / supersample_h2 (4:2:2) of the top-left cw x ch window of the
                       decoded chroma planes, cw = ceil(width / 2), ch = ceil(height / 2) (4:2:0 only): dst[2c] = a,
                       dst[2c + 1] = avg2 a b, the row below avg2 a c / avg4 a b c d, last column and row repeated
    colour             libjpeg's 16-bit fixed-point form of the JFIF matrix (ITU-T T.871), >> arithmetic
    sub-sampling       Planar_444.subsample_hv2 (avg4 of the 2 x 2) / subsample_h2 (avg2 of the pair)

sampling is 420, 422, 444 or 400 (luma only: grey, R = G = B = Y).  Three components are always Y, Cb, Cr."""
import numpy as np

SAMPLINGS = (420, 422, 444, 400)


def ycc_to_rgb(y, cb, cr):
    """uint8 arrays of one shape -> (r, g, b) uint8"""
    y, u, v = np.asarray(y).astype(np.int64), np.asarray(cb).astype(np.int64) - 128, np.asarray(cr).astype(np.int64) - 128
    r = y + ((91881 * v + 32768) >> 16)
    g = y + ((-22554 * u - 46802 * v + 32768) >> 16)
    b = y + ((116130 * u + 32768) >> 16)
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (r, g, b))


def rgb_to_ycc_unclamped(r, g, b):
    """(y, cb, cr) as int64, BEFORE any clamp: every value is in 0 .. 255 for every input (tests/test_rgb_reference.py)"""
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def rgb_to_ycc(r, g, b):
    return tuple(c.astype(np.uint8) for c in rgb_to_ycc_unclamped(r, g, b))


def _avg2(a, b):
    return (a + b + 1) >> 1


def supersample_h2(src):
    """w x h -> 2w x h (planar_444.ml:25-33)"""
    a = np.asarray(src).astype(np.int64)
    b = np.concatenate([a[:, 1:], a[:, -1:]], axis=1)  # the right neighbour; the last column: itself
    out = np.empty((a.shape[0], 2 * a.shape[1]), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = a, _avg2(a, b)
    return out.astype(np.uint8)


def supersample_hv2(src):
    """w x h -> 2w x 2h (planar_444.ml:82-103)"""
    a = np.asarray(src).astype(np.int64)
    b = np.concatenate([a[:, 1:], a[:, -1:]], axis=1)
    c = np.concatenate([a[1:], a[-1:]], axis=0)        # the row below; the last row: itself
    d = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((2 * a.shape[0], 2 * a.shape[1]), dtype=np.int64)
    out[0::2, 0::2], out[0::2, 1::2] = a, _avg2(a, b)
    out[1::2, 0::2], out[1::2, 1::2] = _avg2(a, c), (a + b + c + d + 2) >> 2
    return out.astype(np.uint8)


def subsample_h2(src):
    """2w x h -> w x h (planar_444.ml:18-23)"""
    a = np.asarray(src).astype(np.int64)
    return _avg2(a[:, 0::2], a[:, 1::2]).astype(np.uint8)


def subsample_hv2(src):
    """2w x 2h -> w x h (planar_444.ml:69-80)"""
    a = np.asarray(src).astype(np.int64)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def chroma_window(sampling, width, height):
    """(cw, ch): the chroma samples the image of a width x height frame is made from"""
    return (width if sampling == 444 else (width + 1) // 2, (height + 1) // 2 if sampling == 420 else height)


def full_size_chroma(plane, sampling, width, height):
    """a decoded chroma plane (at least the window) -> width x height"""
    cw, ch = chroma_window(sampling, width, height)
    win = np.asarray(plane)[:ch, :cw]
    assert win.shape == (ch, cw), (win.shape, ch, cw)
    full = supersample_hv2(win) if sampling == 420 else supersample_h2(win) if sampling == 422 else win
    return full[:height, :width]


def planes_to_rgb(y, cb, cr, sampling, width, height, layout="interleaved"):
    """decoded planes (padded or not; cb / cr ignored for 400) -> uint8 [h, w, 3] (interleaved) or [3, h, w] (planar)"""
    assert sampling in SAMPLINGS
    yy = np.asarray(y)[:height, :width]
    assert yy.shape == (height, width)
    if sampling == 400:
        r = g = b = yy.astype(np.uint8)
    else:
        r, g, b = ycc_to_rgb(yy, full_size_chroma(cb, sampling, width, height), full_size_chroma(cr, sampling, width, height))
    return np.stack([r, g, b], axis=0 if layout == "planar" else 2)


def rgb_to_planes(rgb, sampling, layout="interleaved"):
    """uint8 [h, w, 3] / [3, h, w] -> (y, cb, cr) at the sampling's sizes (cb = cr = None for 400); even width for 422 and
    420, even height for 420 (the encoder's rule)"""
    assert sampling in SAMPLINGS
    rgb = np.asarray(rgb)
    r, g, b = (rgb[0], rgb[1], rgb[2]) if layout == "planar" else (rgb[..., 0], rgb[..., 1], rgb[..., 2])
    h, w = r.shape
    if sampling in (420, 422) and w % 2:
        raise ValueError("odd width")
    if sampling == 420 and h % 2:
        raise ValueError("odd height")
    y, cb, cr = rgb_to_ycc(r, g, b)
    if sampling == 400:
        return y, None, None
    if sampling == 420:
        return y, subsample_hv2(cb), subsample_hv2(cr)
    if sampling == 422:
        return y, subsample_h2(cb), subsample_h2(cr)
    return y, cb, cr


def write_ppm(path, rgb):
    """uint8 [h, w, 3] -> binary PPM (P6)"""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())
