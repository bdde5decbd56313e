"""hvc_rgb_resize_mixed_opts on the GPU: a box and a mirror flag per image, and the typed output of k_resize_v_mixed_lut
(include/hvc_jpeg.h, Resizing: Box, Mirror, Typed output; csrc/hvc_resize.hip).  Every comparison is exact equality against
tools/resize_reference.py resize_box / apply_lut (Pillow's Image.resize(box=...), bit for bit: tests/test_resize_box_reference.py);
buffers are filled with 0xA5 and compared whole.  The shapes are the smallest at which the kernels can go wrong."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import resize_box_cases as bc
import resize_cases as rc
from test_gpu_resize import as_layout, place, run, view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resize_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5

# (w, h, W, H, kind of box, mirror): 24 images of 1 x 1 to 70 x 53 -- down, up, the same size (a box or a mirror still runs the
# axis), one axis the same, every kind of box of tests/resize_box_cases.py, a mirror on every other kind
SET = [
    (1, 1, 1, 1, "none", 1), (1, 1, 8, 8, "fraction", 0), (2, 3, 21, 3, "thin", 1), (5, 7, 10, 14, "integer", 0), (5, 7, 5, 7, "whole", 1),
    (17, 9, 7, 9, "left", 0), (17, 9, 17, 9, "none", 0), (17, 9, 17, 18, "top", 1), (17, 9, 34, 18, "fraction", 1), (17, 9, 17, 9, "integer", 0),
    (53, 45, 31, 17, "fraction", 0), (53, 45, 31, 17, "integer", 1), (53, 45, 1, 1, "thin", 0), (53, 45, 53, 45, "right", 1),
    (53, 45, 8, 45, "bottom", 0), (64, 48, 24, 16, "none", 1), (64, 48, 24, 16, "left", 1), (64, 48, 64, 16, "top", 0), (64, 48, 8, 8, "thin", 1),
    (70, 53, 31, 17, "bottom", 1), (70, 53, 70, 53, "whole", 0), (70, 53, 3, 2, "right", 0), (70, 53, 140, 53, "fraction", 1), (70, 53, 1, 53, "integer", 0),
]


def box_of(k):
    w, h, _, _, kind, _ = SET[k]
    return bc.boxes(w, h)[kind]


def spelled(box, w, h):
    """the box as the C call takes it: four values (None: the whole image)"""
    return box if box is not None else (0.0, 0.0, float(w), float(h))


def test_the_set_is_what_it_claims():
    assert len(SET) == 24 and min(s[:2] for s in SET) == (1, 1) and max(s[:2] for s in SET) == (70, 53)
    assert {s[4] for s in SET} == set(bc.boxes(17, 9))
    for kind in ("integer", "fraction", "thin", "left", "top", "right", "bottom"):
        assert {s[5] for s in SET if s[4] == kind} == {0, 1}, kind
    # both axes run with a row window that leaves rows out (the horizontal pass starts below row 0), and axes that only a box
    # or only a mirror makes run
    assert any(rr.row_window(s[1], s[3], "bilinear", box_of(k)[1], box_of(k)[3])[0] > 0 for k, s in enumerate(SET) if box_of(k) is not None)
    assert (17, 9, 17, 9, "integer", 0) in SET and (5, 7, 5, 7, "whole", 1) in SET


@pytest.fixture()
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


_SRC, _WANT = {}, {}


def source(k):
    if k not in _SRC:
        w, h = SET[k][:2]
        _SRC[k] = np.random.default_rng(104729 * k + 7).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return _SRC[k]


def want(k, filt):
    """the definition's image of SET[k], [H, W, 3]: computed once, never changed"""
    if (k, filt) not in _WANT:
        _WANT[k, filt] = rr.resize_box(source(k), SET[k][2], SET[k][3], filt, box_of(k), bool(SET[k][5]))
        _WANT[k, filt].setflags(write=False)
    return _WANT[k, filt]


def filled_source(layout, rows, align):
    s_off, s_str, s_len = place([s[:2] for s in SET], layout, rows, align)
    src = np.full(s_len, 0x3C, dtype=np.uint8)
    for k, s in enumerate(SET):
        view(src, s_off[k], s_str[k], s[0], s[1], layout)[...] = as_layout(source(k), layout)
    return src, s_off, s_str


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("rows", ["tight", "padded"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("filt", rc.FILTERS)
def test_a_box_and_a_mirror_per_image(ctx, filt, layout, rows, device):
    align = "odd" if rows == "tight" else "8"                    # (tight rows at odd offsets: the byte path; padded on 8: dwords)
    src, s_off, s_str = filled_source(layout, rows, align)
    d_off, d_str, d_len = place([s[2:4] for s in SET], layout, rows, align)
    dst = np.full(d_len, FILL, dtype=np.uint8)
    expect = dst.copy()
    for k, s in enumerate(SET):
        view(expect, d_off[k], d_str[k], s[2], s[3], layout)[...] = as_layout(want(k, filt), layout)
    run(ctx, device, src, dst, s_off, [s[0] for s in SET], [s[1] for s in SET], d_off, [s[2] for s in SET], [s[3] for s in SET],
        filter=filt, layout=layout, src_row_strides=s_str if rows == "padded" else None, dst_row_strides=d_str if rows == "padded" else None,
        boxes=[spelled(box_of(k), s[0], s[1]) for k, s in enumerate(SET)], mirror=[s[5] for s in SET])
    bad = np.flatnonzero(dst != expect)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), [k for k in range(len(SET)) if d_off[k] <= bad[0]][-1])


def raw_call(ctx, fn, src, dst, s_off, d_off, layout, filt, opts=()):
    """the C entry point itself on host memory: fn = "hvc_rgb_resize_mixed" (opts: ()) or "..._opts" (opts: (pointer or None,))"""
    import video_coding_amd as hvc
    n = len(SET)
    ints = lambda v: (C.c_int * n)(*v)
    sizes = lambda v: (C.c_size_t * n)(*v)
    return getattr(hvc.lib(), fn)(ctx._h, src.ctypes.data, sizes(s_off), None, ints([s[0] for s in SET]), ints([s[1] for s in SET]), n, dst.ctypes.data,
                                  sizes(d_off), None, ints([s[2] for s in SET]), ints([s[3] for s in SET]), hvc.hvc.HVC_RGB[layout],
                                  hvc.hvc.HVC_RESIZE[filt], 0, *opts)


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_without_options_it_is_the_call_as_it_was(ctx, layout):
    """opts NULL, and an all-zero block: byte for byte hvc_rgb_resize_mixed"""
    import video_coding_amd as hvc
    src, s_off, _ = filled_source(layout, "tight", "8")
    d_off, _, d_len = place([s[2:4] for s in SET], layout, "tight", "8")
    outs = []
    for fn, opts in (("hvc_rgb_resize_mixed", ()), ("hvc_rgb_resize_mixed_opts", (None,)), ("hvc_rgb_resize_mixed_opts", (C.byref(hvc.hvc.ResizeOpts()),))):
        dst = np.full(d_len, FILL, dtype=np.uint8)
        assert raw_call(ctx, fn, src, dst, s_off, d_off, layout, "bicubic", opts) == 0
        outs.append(dst)
    assert np.array_equal(outs[1], outs[0]) and np.array_equal(outs[2], outs[0])
    k = 10
    got = view(outs[0], d_off[k], 0, SET[k][2], SET[k][3], layout)
    assert np.array_equal(got, as_layout(rr.resize(source(k), SET[k][2], SET[k][3], "bicubic"), layout))


# ---- typed output -------------------------------------------------------------------------------------------------------------
# (w, h, W, H, kind of box, mirror).  Interleaved rows of 3 W samples, planar rows of W: the tail lane of a row has
# (samples % 4) left -- 258, 513, 51, 93, 30, 3, 72 samples interleaved (2, 1, 3, 1, 2, 3, 0) and 86, 171, 17, 31, 10, 1, 24 planar
# (2, 3, 1, 3, 2, 1, 0).  Interleaved W = 86 and 171: rows of 65 and 129 lanes, 2 and 3 units whose first lanes start at
# channels 64 % 3 = 1 and 128 % 3 = 2.  17 x 9 -> 17 x 9 without a box: both axes skipped, the identity table.
TYPED = [(86, 5, 86, 3, "none", 0), (171, 4, 171, 2, "none", 0), (17, 9, 17, 9, "none", 0), (53, 45, 31, 17, "fraction", 1), (5, 7, 10, 14, "integer", 0),
         (1, 1, 1, 1, "none", 1), (64, 48, 24, 16, "left", 1)]


def typed_units(layout):
    per_row = lambda W: -(-(-(-(W if layout == "planar" else 3 * W) // 4)) // 64)
    return sum(per_row(s[2]) * s[3] * (3 if layout == "planar" else 1) for s in TYPED)


def test_the_typed_set_is_what_it_claims():
    assert typed_units("interleaved") % 4 != 0 and typed_units("planar") % 4 != 0     # the last workgroup has spare units
    assert {(3 * s[2]) % 4 for s in TYPED} == {0, 1, 2, 3} and {s[2] % 4 for s in TYPED} == {0, 1, 2, 3}
    assert -(-3 * 86 // 4) == 65 and -(-3 * 171 // 4) == 129
    # in the same launch: a unit with a single active lane (1 x 1 in both layouts, the 65th lane of W = 86 interleaved) and rows
    # of one unit (groups == 1)
    assert any(s[2] == 1 for s in TYPED) and any(-(-3 * s[2] // 4) <= 64 for s in TYPED)


_TSRC, _TWANT = {}, {}


def typed_want(k, filt):
    if (k, filt) not in _TWANT:
        w, h, W, H, kind, mirror = TYPED[k]
        if k not in _TSRC:
            _TSRC[k] = np.random.default_rng(31337 * k + 5).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        _TWANT[k, filt] = rr.resize_box(_TSRC[k], W, H, filt, bc.boxes(w, h)[kind], bool(mirror))
        _TWANT[k, filt].setflags(write=False)
    return _TSRC[k], _TWANT[k, filt]


def put_typed(buf, off, stride, img, layout):
    """the typed image [H, W, 3] into a buffer of bytes, row by row, as raw bits"""
    rows = (np.ascontiguousarray(img.transpose(2, 0, 1)).reshape(-1, img.shape[1]) if layout == "planar"
            else np.ascontiguousarray(img).reshape(img.shape[0], -1))
    for r, row in enumerate(rows):
        raw = np.ascontiguousarray(row).view(np.uint8)
        buf[off + r * stride:off + r * stride + raw.size] = raw


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("align", ["on", "off"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("elem", [2, 4])
def test_typed_output_through_a_random_table(ctx, elem, layout, align, device):
    """align on: every destination row starts on 4 * elem bytes (rows padded to it): the 8- / 16-byte stores, element stores only
    in a row's tail lane; off: records at an odd multiple of elem and tight rows: element stores throughout.  The table is
    random bits, so that no formula can hide an indexing slip."""
    filt = rc.FILTERS[(elem // 2 + (layout == "planar") + (align == "on")) % 3]
    lut = np.random.default_rng(elem * 10 + (layout == "planar")).integers(0, 1 << (8 * elem), size=(3, 256), dtype=np.uint64).astype({2: np.uint16, 4: np.uint32}[elem])
    s_off, _, s_len = place([s[:2] for s in TYPED], layout, "tight", "8")
    src = np.full(s_len, 0x3C, dtype=np.uint8)
    d_off, d_str, at = [], [], 0
    for w, h, W, H, _, _ in TYPED:
        samples = W if layout == "planar" else 3 * W
        if align == "on":
            stride, at = -(-samples // 4) * 4 * elem + 4 * elem * (W % 2), -(-at // 64) * 64
        else:
            stride, at = samples * elem, -(-at // (4 * elem)) * 4 * elem + elem
        d_off.append(at)
        d_str.append(stride)
        at += stride * H * (3 if layout == "planar" else 1) + 6
    dst = np.full(at + 32, FILL, dtype=np.uint8)
    expect = dst.copy()
    for k, (w, h, W, H, kind, mirror) in enumerate(TYPED):
        img, out8 = typed_want(k, filt)
        view(src, s_off[k], 0, w, h, layout)[...] = as_layout(img, layout)
        put_typed(expect, d_off[k], d_str[k], rr.apply_lut(out8, lut), layout)
    run(ctx, device, src, dst, s_off, [s[0] for s in TYPED], [s[1] for s in TYPED], d_off, [s[2] for s in TYPED], [s[3] for s in TYPED],
        filter=filt, layout=layout, dst_row_strides=d_str, boxes=[spelled(bc.boxes(s[0], s[1])[s[4]], s[0], s[1]) for s in TYPED],
        mirror=[s[5] for s in TYPED], lut=lut)
    bad = np.flatnonzero(dst != expect)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), [k for k in range(len(TYPED)) if d_off[k] <= bad[0]][-1])


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_dtype_with_mean_and_std_is_torchs_normalised_tensor(ctx, dtype):
    """the public form: dtype= with mean= / std= writes torchvision's ToTensor() + Normalize() of the resized image, bit for bit"""
    import torch
    import video_coding_amd as hvc
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    img = rc.noise(53, 45)
    W, H, box = 24, 16, (3.5, 2.25, 40.0, 30.5)
    esz = hvc.hvc.ELEM_BYTES[dtype]
    dst = np.full(3 * W * H * esz + 8, FILL, dtype=np.uint8)
    planes = np.ascontiguousarray(img.transpose(2, 0, 1)).reshape(-1)           # (planar: the source's planes, as the destination's)
    ctx.rgb_resize_mixed(planes, [0], [53], [45], dst, [0], [W], [H], filter="bilinear", layout="planar", boxes=[box], mirror=[1],
                         dtype=dtype, mean=mean, std=std)
    want8 = torch.from_numpy(rr.resize_box(img, W, H, "bilinear", box, True).transpose(2, 0, 1).copy())
    want = ((want8.float() / 255 - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]).to(getattr(torch, dtype))
    got = torch.from_numpy(dst[:3 * W * H * esz]).view(getattr(torch, dtype)).reshape(3, H, W)
    bits = {4: torch.int32, 2: torch.int16}[esz]
    assert torch.equal(got.view(bits), want.view(bits)) and (dst[3 * W * H * esz:] == FILL).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_leave_the_output_untouched(ctx, device):
    import video_coding_amd as hvc
    img = rc.noise(40, 24)
    src = img.reshape(-1).copy()
    lut = np.zeros((3, 256), np.uint16)
    nan = float("nan")
    cases = [dict(boxes=[(0, 0, 40.5, 24)]), dict(boxes=[(0, 0, 40, 25)]), dict(boxes=[(-1, 0, 40, 24)]), dict(boxes=[(0, -0.5, 40, 24)]),
             dict(boxes=[(7, 0, 7, 24)]), dict(boxes=[(0, 12, 40, 11)]), dict(boxes=[(nan, 0, 40, 24)]), dict(boxes=[(0, 0, float("inf"), 24)]),
             dict(lut=lut, dst_row_strides=[119])]                # a typed row of 120 bytes
    for kw in cases:
        dst = np.full(4096, FILL, np.uint8)
        with pytest.raises(hvc.HvcError) as e:
            run(ctx, device, src, dst, [0], [40], [24], [0], [20], [12], **kw)
        assert e.value.code == -1 and (dst == FILL).all(), kw
    # the option block itself: an out_elem that is none of 0, 2, 4, and a typed output without a table
    for out_elem, table in ((1, lut), (3, lut), (8, lut), (-2, lut), (2, None), (4, None)):
        o = hvc.hvc.ResizeOpts()
        o.out_elem, o.lut = out_elem, table.ctypes.data if table is not None else None
        dst = np.full(4096, FILL, np.uint8)
        one = lambda v, t=C.c_int: (t * 1)(v)
        r = hvc.lib().hvc_rgb_resize_mixed_opts(ctx._h, src.ctypes.data, one(0, C.c_size_t), None, one(40), one(24), 1, dst.ctypes.data, one(0, C.c_size_t),
                                                None, one(20), one(12), 0, 1, 0, C.byref(o))
        assert r == -1 and (dst == FILL).all(), (out_elem, table is None)
    # and the same image without the fault goes through: the context is as it was
    dst = np.full(4096, FILL, np.uint8)
    run(ctx, device, src, dst, [0], [40], [24], [0], [20], [12], filter="box", boxes=[(1.5, 2.0, 30.0, 20.5)], mirror=[1])
    assert np.array_equal(dst[:720].reshape(12, 20, 3), rr.resize_box(img, 20, 12, "box", (1.5, 2.0, 30.0, 20.5), True)) and (dst[720:] == FILL).all()

