"""Resizing an 8-bit image, in numpy -- the definition csrc/hvc_resize.hip and csrc/hvc_resize_plan.cpp are tested against
(include/hvc_jpeg.h, Resizing): Pillow's Image.resize on 8-bit images, bit for bit, for the filters box, bilinear and
bicubic.  Stands alone: numpy only, no import from the library or from the test oracle.

    coefficients   per axis n_in -> n_out, in IEEE double with one rounding per operation (every product and sum is a numpy
                   call of its own: nothing can be fused), then 22-bit integer taps
    a pass         clip_0_255((2^21 + SUM k[i] * in[xmin + i]) >> 22), arithmetic shift, 8-bit samples out
    order          horizontal first (to an 8-bit intermediate of out_w x h_in), then vertical; an axis with n_out == n_in
                   is skipped

Hamming and Lanczos are left out: they need cos / sin, whose last bit differs between C libraries."""
import numpy as np

FILTERS = ("box", "bilinear", "bicubic")
SUPPORT = {"box": 0.5, "bilinear": 1.0, "bicubic": 2.0}
PRECISION_BITS = 22


def _box(x):
    return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, np.subtract(1.0, x), 0.0)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    # ((a + 2) |x| - (a + 3)) x^2 + 1: ((t * x) * x) + 1, as the C expression associates
    near = np.add(np.multiply(np.multiply(np.subtract(np.multiply(a + 2.0, x), a + 3.0), x), x), 1.0)
    # (((|x| - 5) |x| + 8) |x| - 4) a
    far = np.multiply(np.subtract(np.multiply(np.add(np.multiply(np.subtract(x, 5.0), x), 8.0), x), 4.0), a)
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


_FILTER = {"box": _box, "bilinear": _bilinear, "bicubic": _bicubic}


def coefficients(n_in, n_out, filter):
    """The taps of one axis: (xmin[n_out], count[n_out], taps[n_out][kmax]) as int64 arrays; taps[xx][i] for i >= count[xx]
    are 0.  kmax = max(count)."""
    if filter not in _FILTER:
        raise ValueError("unknown filter %r" % (filter,))
    if n_in < 1 or n_out < 1:
        raise ValueError("sizes start at 1")
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ss = 1.0 / fs
    center = np.multiply(np.add(np.arange(n_out, dtype=np.float64), 0.5), scale)
    # (int) truncates towards zero
    xmin = np.maximum(np.trunc(np.add(np.subtract(center, support), 0.5)).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(np.add(np.add(center, support), 0.5)).astype(np.int64), n_in)
    count = xmax - xmin
    kmax = int(count.max())
    i = np.arange(kmax, dtype=np.int64)[None, :]
    live = i < count[:, None]
    # f((i + xmin - center + 0.5) * ss): i + xmin is an integer (exact), then - center, + 0.5, * ss
    x = np.multiply(np.add(np.subtract((i + xmin[:, None]).astype(np.float64), center[:, None]), 0.5), ss)
    w = np.where(live, _FILTER[filter](x), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1]            # in index order (the zeros behind `count` change nothing)
    w = np.where((ww != 0.0)[:, None], np.divide(w, np.where(ww != 0.0, ww, 1.0)[:, None]), w)
    scaled = np.multiply(w, float(1 << PRECISION_BITS))
    taps = np.where(w < 0.0, np.trunc(np.subtract(scaled, 0.5)), np.trunc(np.add(scaled, 0.5))).astype(np.int64)
    taps[~live] = 0
    return xmin, count, taps


def _pass_rows(src, n_out, filter):
    """src [rows, n_in, c] uint8 -> [rows, n_out, c] uint8 along axis 1"""
    xmin, count, taps = coefficients(src.shape[1], n_out, filter)
    out = np.empty((src.shape[0], n_out, src.shape[2]), dtype=np.uint8)
    s = src.astype(np.int64)
    for xx in range(n_out):
        n = int(count[xx])
        acc = (s[:, xmin[xx]:xmin[xx] + n, :] * taps[xx, :n][None, :, None]).sum(axis=1) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max(initial=0) < (1 << 31)       # the accumulator is an int32 on the GPU
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, W, H, filter="bilinear"):
    """img [h, w, c] (or [h, w]) uint8 -> [H, W, c] (or [H, W]) uint8"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("an 8-bit image of [h, w] or [h, w, c]")
    if filter not in _FILTER:
        raise ValueError("unknown filter %r" % (filter,))
    if W < 1 or H < 1 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("sizes start at 1")
    cur = img.reshape(img.shape[0], img.shape[1], -1)
    if W != cur.shape[1]:
        cur = _pass_rows(cur, W, filter)
    if H != cur.shape[0]:
        cur = _pass_rows(cur.transpose(1, 0, 2), H, filter).transpose(1, 0, 2)
    return np.ascontiguousarray(cur).reshape((H, W) + img.shape[2:])


def resize_planar(planes, W, H, filter="bilinear"):
    """planes [c, h, w] uint8 -> [c, H, W]: every plane is a one-channel image of its own"""
    planes = np.asarray(planes)
    return np.stack([resize(p, W, H, filter) for p in planes])


def max_abs_tap_sum(n_in, n_out, filter):
    """the largest SUM |k| over the output positions of one axis: 255 * it + 2^21 must stay below 2^31"""
    _, _, taps = coefficients(n_in, n_out, filter)
    return int(np.abs(taps).sum(axis=1).max())


# ---- the box, the mirror and the typed output (include/hvc_jpeg.h, Resizing: Box, Mirror, Typed output) ----

def coefficients_box(n_in, n_out, filter, in0=0.0, in1=None):
    """The taps of one axis that resamples the window [in0, in1) of n_in samples to n_out: Pillow's Image.resize(box=...).  in0,
    in1 are IEEE single values (in1 None: n_in); the span is subtracted in SINGLE precision and then widened, the centre is
    (double)in0 + (xx + 0.5) * scale; everything else is `coefficients`.  Taps may reach outside the window, never outside the
    samples.  Returns (xmin, count, taps) as `coefficients` does."""
    if filter not in _FILTER:
        raise ValueError("unknown filter %r" % (filter,))
    if n_in < 1 or n_out < 1:
        raise ValueError("sizes start at 1")
    in0 = np.float32(in0)
    in1 = np.float32(n_in if in1 is None else in1)
    if not (np.isfinite(in0) and np.isfinite(in1)):
        raise ValueError("a box of finite values")
    if in0 < 0 or in1 > n_in:
        raise ValueError("the box leaves the image")
    span = np.subtract(in1, in0, dtype=np.float32)
    if not span > 0:
        raise ValueError("an empty box")
    scale = float(span) / float(n_out)
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ss = 1.0 / fs
    center = np.add(float(in0), np.multiply(np.add(np.arange(n_out, dtype=np.float64), 0.5), scale))
    xmin = np.maximum(np.trunc(np.add(np.subtract(center, support), 0.5)).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(np.add(np.add(center, support), 0.5)).astype(np.int64), n_in)
    count = xmax - xmin
    kmax = max(int(count.max()), 1)
    i = np.arange(kmax, dtype=np.int64)[None, :]
    live = i < count[:, None]
    x = np.multiply(np.add(np.subtract((i + xmin[:, None]).astype(np.float64), center[:, None]), 0.5), ss)
    w = np.where(live, _FILTER[filter](x), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1]
    w = np.where((ww != 0.0)[:, None], np.divide(w, np.where(ww != 0.0, ww, 1.0)[:, None]), w)
    scaled = np.multiply(w, float(1 << PRECISION_BITS))
    taps = np.where(w < 0.0, np.trunc(np.subtract(scaled, 0.5)), np.trunc(np.add(scaled, 0.5))).astype(np.int64)
    taps[~live] = 0
    return xmin, count, taps


def _pass_rows_box(src, n_out, filter, in0, in1):
    """_pass_rows under a window: src [rows, n_in, c] uint8 -> [rows, n_out, c] uint8 along axis 1"""
    xmin, count, taps = coefficients_box(src.shape[1], n_out, filter, in0, in1)
    out = np.empty((src.shape[0], n_out, src.shape[2]), dtype=np.uint8)
    s = src.astype(np.int64)
    for xx in range(n_out):
        n = int(count[xx])
        acc = (s[:, xmin[xx]:xmin[xx] + n, :] * taps[xx, :n][None, :, None]).sum(axis=1) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max(initial=0) < (1 << 31)
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def axis_skipped(n_in, n_out, in0, in1):
    """an axis is skipped iff n_out == n_in and the window is the whole axis"""
    return n_out == n_in and np.float32(in0) == 0 and np.float32(in1) == n_in


def resize_box(img, W, H, filter="bilinear", box=None, mirror=False):
    """img [h, w, c] (or [h, w]) uint8 -> [H, W, c] (or [H, W]) uint8: Image.resize((W, H), filter, box=box), then (mirror)
    .transpose(FLIP_LEFT_RIGHT).  box = (x0, y0, x1, y1) in the image's coordinates, IEEE single, fractional values allowed;
    None: the whole image.  The horizontal pass runs over every source row here: the rows outside the vertical pass's window
    are never read again, so the result is that of the row window (hvc_jpeg.h)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("an 8-bit image of [h, w] or [h, w, c]")
    if filter not in _FILTER:
        raise ValueError("unknown filter %r" % (filter,))
    if W < 1 or H < 1 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("sizes start at 1")
    h, w = img.shape[:2]
    x0, y0, x1, y1 = (0.0, 0.0, float(w), float(h)) if box is None else (np.float32(v) for v in box)
    cur = img.reshape(h, w, -1)
    for lo, hi, n in ((x0, x1, w), (y0, y1, h)):        # both axes are judged before either runs
        coefficients_box(n, 1, filter, lo, hi)
    if not axis_skipped(w, W, x0, x1):
        cur = _pass_rows_box(cur, W, filter, x0, x1)
    if not axis_skipped(h, H, y0, y1):
        cur = _pass_rows_box(cur.transpose(1, 0, 2), H, filter, y0, y1).transpose(1, 0, 2)
    if mirror:
        cur = cur[:, ::-1, :]
    return np.ascontiguousarray(cur).reshape((H, W) + img.shape[2:])


def row_window(n_in, n_out, filter, in0=0.0, in1=None):
    """[first, last) of the source samples the axis reads: [xmin[0], xmin[n_out - 1] + count[n_out - 1]) -- the rows the
    horizontal pass covers when both axes run"""
    xmin, count, _ = coefficients_box(n_in, n_out, filter, in0, in1)
    return int(xmin[0]), int(xmin[-1] + count[-1])


def apply_lut(img, lut, channel_axis=-1):
    """Typed output: sample v of channel c becomes lut[c][v], raw bits.  img: uint8 with 3 channels along channel_axis ([H, W, 3]:
    -1, [3, H, W]: 0); lut: [3, 256] of any 2- or 4-byte element type.  Returns an array of lut's dtype in img's shape."""
    img, lut = np.asarray(img), np.asarray(lut)
    if img.dtype != np.uint8 or lut.shape != (3, 256) or img.shape[channel_axis] != 3:
        raise ValueError("an 8-bit image of 3 channels and a table of [3, 256]")
    moved = np.moveaxis(img, channel_axis, 0)
    out = np.stack([lut[c][moved[c]] for c in range(3)])
    return np.ascontiguousarray(np.moveaxis(out, 0, channel_axis))


def normalize_lut(mean, std, dtype=np.float32):
    """The table hvc_normalize_lut makes, in numpy: ((float)v / 255.0f - mean[c]) / std[c] in IEEE single, one rounding per
    operation, then (float16) one round-to-nearest-even conversion.  [3, 256] of dtype (float32 or float16)."""
    v = np.arange(256, dtype=np.float32)[None, :]
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1)
    return np.divide(np.subtract(np.divide(v, np.float32(255.0)), m), s).astype(dtype)
