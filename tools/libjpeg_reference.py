"""The decoder of include/hvc_jpeg.h ("Bit-exact to libjpeg": hvc_set_arithmetic HVC_ARITH_LIBJPEG) in numpy int64: the
checker of k_islow and k_ycc_to_rgb_fancy.  Pure numpy, no library of the project: what it computes is held against
libjpeg-turbo (through PIL) by tests/test_libjpeg_reference.py, and the GPU against it by tests/test_gpu_libjpeg.py.

    block stage        libjpeg's jidctint.c ("islow"): two passes of one 13-bit fixed-point step, descaled by 11 and 18
    full-size chroma   libjpeg's "fancy" triangle filter (jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample) of the
                       top-left cw x ch window of the chroma planes; windows at most 2 samples wide are replicated
    colour             libjpeg's 16-bit fixed-point form of the JFIF matrix, as in tools/rgb_reference.py

Coefficients are in the C ABI's layout: [..., 64] int16 in zig-zag order with the DC absolute; tables are 64 entries in
zig-zag order -- the conventions of tools/scaled_reference.py."""
import os
import re

import numpy as np

# natural position (8 * row + col) -> zig-zag position
ZF = np.array([0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40,
               44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36,
               48, 49, 57, 58, 62, 63])

SAMPLINGS = (420, 422, 444, 400)

SPEC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-coding_amd", "csrc", "hvc_islow_spec.h")


def D(x, n):
    return (x + (1 << (n - 1))) >> n


def dequantised(coefs, qtab):
    """[..., 64] zig-zag coefficients x zig-zag table -> d[..., row, col] in natural order.  int64 holds every int16
    coefficient times every 16-bit entry; the passes below go to Python integers where int64 could not hold them."""
    d = np.asarray(coefs).astype(np.int64) * np.asarray(qtab).astype(np.int64).reshape(64)
    return d[..., ZF].reshape(d.shape[:-1] + (8, 8))


def islow_step(v, sh):
    """v[i]: arrays, i = 0..7 -> the eight results"""
    z1 = (v[2] + v[6]) * 4433
    tmp2 = z1 - v[6] * 15137
    tmp3 = z1 + v[2] * 6270
    tmp0 = (v[0] + v[4]) << 13
    tmp1 = (v[0] - v[4]) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    a0, a1, a2, a3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return [D(t10 + a3, sh), D(t11 + a2, sh), D(t12 + a1, sh), D(t13 + a0, sh),
            D(t13 - a0, sh), D(t12 - a1, sh), D(t11 - a2, sh), D(t10 - a3, sh)]


def islow_blocks(coefs, qtab):
    """[..., 64] coefficients -> [..., 8, 8] uint8 samples"""
    d = dequantised(coefs, qtab)
    if np.abs(d).max(initial=0) >= 1 << 24:  # beyond int64 after two passes: unbounded integers
        d = d.astype(object)
    cols = [islow_step([d[..., r, c] for r in range(8)], 11) for c in range(8)]   # cols[c][r]
    rows = [islow_step([cols[c][r] for c in range(8)], 18) for r in range(8)]     # rows[r][c]
    x = np.stack([np.stack(rows[r], axis=-1) for r in range(8)], axis=-2)
    return np.clip(x + 128, 0, 255).astype(np.uint8)


def islow_plane(coefs, qtab, bw, bh):
    """one component plane: [bh][bw][64] coefficients -> [bh * 8][bw * 8] uint8"""
    b = islow_blocks(np.asarray(coefs).reshape(bh, bw, 64), qtab)
    return b.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def spec_constants():
    """the plain-integer #define's of hvc_islow_spec.h as {name: int}"""
    out = {}
    for name, val in re.findall(r"^#define\s+(HVC_IS_\w+)\s+(\d+)u?\s*$", open(SPEC).read(), flags=re.M):
        out[name] = int(val)
    return out


def guard_sum(coefs, qtab):
    """[..., 64] coefficients -> S = the sum of |d[k]| over the block"""
    return np.abs(dequantised(coefs, qtab)).sum(axis=(-1, -2))


def takes_int32_path(coefs, qtab):
    """[..., 64] coefficients -> bool [...]: the block passes the guard of hvc_islow_spec.h"""
    return guard_sum(coefs, qtab) <= spec_constants()["HVC_IS_GUARD_SUM"]


# ---- chroma to full size
def replicate(win, fx, fy):
    return np.repeat(np.repeat(np.asarray(win), fy, axis=0), fx, axis=1)


def fancy_h2(win):
    """cw x ch -> 2 cw x ch (4:2:2)"""
    s = np.asarray(win).astype(np.int64)
    cw = s.shape[1]
    if cw <= 2:
        return replicate(win, 2, 1).astype(np.uint8)
    out = np.empty((s.shape[0], 2 * cw), dtype=np.int64)
    out[:, 2::2] = (3 * s[:, 1:] + s[:, :-1] + 1) >> 2
    out[:, 1:2 * cw - 1:2] = (3 * s[:, :-1] + s[:, 1:] + 2) >> 2
    out[:, 0], out[:, -1] = s[:, 0], s[:, -1]
    return out.astype(np.uint8)


def fancy_hv2(win):
    """cw x ch -> 2 cw x 2 ch (4:2:0)"""
    s = np.asarray(win).astype(np.int64)
    ch, cw = s.shape
    if cw <= 2:
        return replicate(win, 2, 2).astype(np.uint8)
    up = np.concatenate([s[:1], s[:-1]], axis=0)    # s[max(r - 1, 0)]
    down = np.concatenate([s[1:], s[-1:]], axis=0)  # s[min(r + 1, ch - 1)]
    t = np.empty((2 * ch, cw), dtype=np.int64)
    t[0::2], t[1::2] = 3 * s + up, 3 * s + down
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    out[:, 2::2] = (3 * t[:, 1:] + t[:, :-1] + 8) >> 4
    out[:, 1:2 * cw - 1:2] = (3 * t[:, :-1] + t[:, 1:] + 7) >> 4
    out[:, 0], out[:, -1] = (4 * t[:, 0] + 8) >> 4, (4 * t[:, -1] + 7) >> 4
    return out.astype(np.uint8)


def chroma_window(sampling, width, height):
    """(cw, ch): the chroma samples the image of a width x height frame is made from"""
    return (width if sampling == 444 else (width + 1) // 2, (height + 1) // 2 if sampling == 420 else height)


def full_size_chroma(plane, sampling, width, height):
    """a decoded chroma plane (at least the window) -> width x height"""
    cw, ch = chroma_window(sampling, width, height)
    win = np.asarray(plane)[:ch, :cw]
    assert win.shape == (ch, cw), (win.shape, ch, cw)
    full = fancy_hv2(win) if sampling == 420 else fancy_h2(win) if sampling == 422 else win
    return full[:height, :width]


def ycc_to_rgb(y, cb, cr):
    """uint8 arrays of one shape -> (r, g, b) uint8"""
    y, u, v = np.asarray(y).astype(np.int64), np.asarray(cb).astype(np.int64) - 128, np.asarray(cr).astype(np.int64) - 128
    r = y + ((91881 * v + 32768) >> 16)
    g = y + ((-22554 * u - 46802 * v + 32768) >> 16)
    b = y + ((116130 * u + 32768) >> 16)
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (r, g, b))


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


def record_planes(coefs, qtabs, planes):
    """a frame's coefficient record (component planes back to back) -> its decoded planes; planes = [(bw, bh, table index)]"""
    coefs, qtabs = np.asarray(coefs).reshape(-1), np.asarray(qtabs).reshape(-1, 64)
    out, at = [], 0
    for bw, bh, t in planes:
        out.append(islow_plane(coefs[at:at + bw * bh * 64], qtabs[t], bw, bh))
        at += bw * bh * 64
    assert at == coefs.size, (at, coefs.size)
    return out


def record_to_rgb(coefs, qtabs, planes, sampling, width, height, layout="interleaved"):
    """a frame's coefficient record -> the RGB image of the file"""
    p = record_planes(coefs, qtabs, planes)
    return planes_to_rgb(p[0], p[1] if len(p) > 1 else None, p[2] if len(p) > 2 else None, sampling, width, height, layout)
