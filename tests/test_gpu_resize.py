"""Resizing on the GPU: hvc_rgb_resize_mixed -- one launch of k_resize_h_mixed and one of k_resize_v_mixed over a SET of images of
different sizes, each to a size of its own.  Every comparison is exact equality against tools/resize_reference.py (Pillow's
Image.resize, bit for bit: tests/test_resize_reference.py); buffers are compared whole over a fill of 0xA5."""
import os
import sys

import numpy as np
import pytest

import resize_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resize_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5

# (w, h, W, H): the issue's inputs, each to a size of its own -- 1 x 1, 8 x 8, 31 x 17, 24 x 16, 224 x 224, the same size, one
# axis the same, 2x, and the long-tap cases 480 x 320 -> 1 x 1 and -> 3 x 2 -- and the images that give each pass its lane counts
SET = [
    (1, 1, 8, 8), (2, 3, 21, 3), (5, 7, 10, 14), (17, 9, 7, 9), (53, 45, 31, 17), (64, 48, 24, 16), (97, 51, 5, 17),
    (100, 37, 100, 37), (480, 320, 224, 224), (480, 320, 1, 1), (480, 320, 3, 2), (64, 48, 8, 8), (53, 45, 1, 1), (17, 9, 17, 18),
    # horizontal: W * h lanes -- 1, 64, 65, 257 (63: 2 x 3 -> 21 x 3 and 17 x 9 -> 7 x 9; 255: 97 x 51 -> 5 x 17)
    (5, 1, 1, 1), (10, 8, 8, 8), (9, 13, 5, 13), (300, 1, 257, 1),
    # vertical, interleaved: ceil(3 W / 4) lanes per row -- 1, 63, 64, 65, 255, 257
    (1, 5, 1, 2), (84, 7, 84, 3), (85, 7, 85, 3), (86, 7, 86, 3), (340, 4, 340, 2), (342, 4, 342, 2),
    # vertical, planar: ceil(W / 4) lanes per row -- 63, 64, 65, 255, 257 (1: 1 x 5 -> 1 x 2)
    (252, 3, 252, 2), (256, 3, 256, 2), (258, 3, 258, 2), (1020, 2, 1020, 1), (1026, 2, 1026, 1),
]
EDGES = {1, 63, 64, 65, 255, 257}


def lanes_of(layout):
    """the lane counts each pass meets, by the mapping of csrc/hvc_resize_plan.h"""
    h_lanes, v_lanes = set(), set()
    for w, h, W, H in SET:
        if W != w:
            h_lanes.add(W * h)
        if H != h or W == w:
            v_lanes.add(-(-(W if layout == "planar" else 3 * W) // 4))
    return h_lanes, v_lanes


def test_the_set_meets_every_lane_count():
    for layout in ("interleaved", "planar"):
        h_lanes, v_lanes = lanes_of(layout)
        assert EDGES <= h_lanes, (layout, sorted(EDGES - h_lanes))
        assert EDGES <= v_lanes, (layout, sorted(EDGES - v_lanes))
    assert max(rr.coefficients(480, 1, "bicubic")[1]) == 480 and max(rr.coefficients(320, 2, "bilinear")[1]) == 240   # several hundred taps


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
        _SRC[k] = np.random.default_rng(7919 * k + 13).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return _SRC[k]


def want(k, filt):
    """the definition's image of SET[k], [H, W, 3]: computed once, never changed"""
    if (k, filt) not in _WANT:
        _WANT[k, filt] = rr.resize(source(k), SET[k][2], SET[k][3], filt)
        _WANT[k, filt].setflags(write=False)
    return _WANT[k, filt]


def view(buf, off, stride, w, h, layout):
    import video_coding_amd as hvc
    return hvc.hvc.rgb_view(buf, off, stride, w, h, layout)


def place(sizes, layout, rows, align):
    """offsets and row strides of images of these (w, h): `align` odd = every record at an odd offset (padded rows: an odd
    stride too -- the byte path), 8 = offsets (and padded strides) on 8 bytes (the dword path)"""
    offs, strides, at = [], [], 3 if align == "odd" else 0
    for w, h in sizes:
        tight = w if layout == "planar" else 3 * w
        stride = tight
        if rows == "padded":
            stride = (tight + 5) | 1 if align == "odd" else (tight + 15) & ~7
        if align == "odd":
            at |= 1
        else:
            at = (at + 7) & ~7
        offs.append(at)
        strides.append(stride)
        at += stride * h * (3 if layout == "planar" else 1) + 2
    return offs, strides, at + 8


def as_layout(img, layout):
    return np.ascontiguousarray(img.transpose(2, 0, 1)) if layout == "planar" else img


def run(ctx, device, src, dst, *args, **kw):
    """the call on host buffers or on device copies of them; dst is updated in place"""
    if not device:
        ctx.rgb_resize_mixed(src, args[0], args[1], args[2], dst, *args[3:], **kw)
        return
    import torch
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)   # order after torch's copies
    try:
        ctx.rgb_resize_mixed(d_src, args[0], args[1], args[2], d_dst, *args[3:], **kw)
    finally:   # (a refused call too: what the device buffer holds afterwards is what the test looks at)
        ctx.synchronize()
        ctx.reset_stream()
        dst[:] = d_dst.cpu().numpy()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("align", ["odd", "8"])
@pytest.mark.parametrize("rows", ["tight", "padded"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("filt", rc.FILTERS)
def test_a_set_of_images_each_to_its_own_size(ctx, filt, layout, rows, align, device):
    n = len(SET)
    s_off, s_str, s_len = place([(w, h) for w, h, _, _ in SET], layout, rows, align)
    d_off, d_str, d_len = place([(W, H) for _, _, W, H in SET], layout, rows, align)
    src = np.full(s_len, 0x3C, dtype=np.uint8)
    dst = np.full(d_len, FILL, dtype=np.uint8)
    expect = dst.copy()
    for k, (w, h, W, H) in enumerate(SET):
        view(src, s_off[k], s_str[k], w, h, layout)[...] = as_layout(source(k), layout)
        view(expect, d_off[k], d_str[k], W, H, layout)[...] = as_layout(want(k, filt), layout)
    run(ctx, device, src, dst, s_off, [s[0] for s in SET], [s[1] for s in SET], d_off, [s[2] for s in SET], [s[3] for s in SET],
        filter=filt, layout=layout, src_row_strides=s_str if rows == "padded" else None, dst_row_strides=d_str if rows == "padded" else None)
    bad = np.flatnonzero(dst != expect)
    assert bad.size == 0, (bad.size, bad[:8].tolist(), [k for k in range(n) if d_off[k] <= bad[0]][-1])


# The smallest set that has, in ONE launch of each pass and in both layouts, a last workgroup with spare units, a unit with a
# single active lane and one unit per row of lanes (groups == 1).  Every image runs one pass only, so the unit counts below
# are exact: horizontal (H == h) 65 lanes of one sample per row and 64 lanes; vertical (W == w) rows of 1, 65 and 3 / 1 lanes.
EDGE_SET = [(5, 65, 1, 65), (10, 8, 8, 8), (1, 5, 1, 2), (86, 7, 86, 3), (258, 3, 258, 2), (4, 3, 4, 2)]
GUARD = 4096


def edge_units(layout):
    """(units of the horizontal pass, units of the vertical pass, lane counts of a horizontal image / of a vertical row)"""
    planes = 3 if layout == "planar" else 1
    hu = vu = 0
    lanes = set()
    for w, h, W, H in EDGE_SET:
        assert (W != w) != (H != h)
        if W != w:
            hu += planes * -(-(W * h) // 64)
            lanes.add(W * h)
        else:
            row = -(-(W if layout == "planar" else 3 * W) // 4)
            vu += planes * H * -(-row // 64)
            lanes.add(row)
    return hu, vu, lanes


@pytest.mark.parametrize("align", ["odd", "8"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_spare_units_a_single_active_lane_and_one_unit_per_row(ctx, layout, align):
    hu, vu, lanes = edge_units(layout)
    assert hu % 4 and vu % 4 and {1, 65} <= lanes, (hu, vu, lanes)
    s_off, _, s_len = place([(w, h) for w, h, _, _ in EDGE_SET], layout, "tight", align)
    d_off, _, d_len = place([(W, H) for _, _, W, H in EDGE_SET], layout, "tight", align)
    src = np.full(s_len, 0x3C, dtype=np.uint8)
    dst = np.full(d_len + GUARD, FILL, dtype=np.uint8)
    expect = dst.copy()
    for k, (w, h, W, H) in enumerate(EDGE_SET):
        img = np.random.default_rng(4001 + k).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        view(src, s_off[k], w if layout == "planar" else 3 * w, w, h, layout)[...] = as_layout(img, layout)
        view(expect, d_off[k], W if layout == "planar" else 3 * W, W, H, layout)[...] = as_layout(rr.resize(img, W, H, "bilinear"), layout)
    run(ctx, True, src, dst, s_off, [s[0] for s in EDGE_SET], [s[1] for s in EDGE_SET], d_off, [s[2] for s in EDGE_SET],
        [s[3] for s in EDGE_SET], filter="bilinear", layout=layout)
    bad = np.flatnonzero(dst != expect)
    assert bad.size == 0, (bad.size, bad[:8].tolist())


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_constant_images_and_the_checkerboard_under_bicubic(ctx, device):
    imgs = [np.zeros((9, 17, 3), np.uint8), np.full((9, 17, 3), 255, np.uint8), rc.checkerboard(53, 45), rc.checkerboard(53, 45),
            rc.checkerboard(53, 45), np.full((9, 17, 3), 255, np.uint8)]
    outs = [(31, 17), (34, 18), (106, 90), (31, 17), (24, 16), (8, 8)]
    layout = "planar" if device else "interleaved"
    s_off, _, s_len = place([(i.shape[1], i.shape[0]) for i in imgs], layout, "tight", "8")
    d_off, _, d_len = place(outs, layout, "tight", "8")
    src, dst = np.zeros(s_len, np.uint8), np.full(d_len, FILL, np.uint8)
    expect = dst.copy()
    for k, (img, (W, H)) in enumerate(zip(imgs, outs)):
        view(src, s_off[k], 0, img.shape[1], img.shape[0], layout)[...] = as_layout(img, layout)
        ref = rr.resize(img, W, H, "bicubic")
        view(expect, d_off[k], 0, W, H, layout)[...] = as_layout(ref, layout)
        if k < 2 or k == 5:
            assert (ref == img[0, 0, 0]).all()
    big = rr.resize(imgs[2], 106, 90, "bicubic")
    assert big.min() == 0 and big.max() == 255                     # both sides of the clip
    run(ctx, device, src, dst, s_off, [i.shape[1] for i in imgs], [i.shape[0] for i in imgs], d_off, [o[0] for o in outs], [o[1] for o in outs],
        filter="bicubic", layout=layout)
    assert np.array_equal(dst, expect)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_uniform_tensor_with_one_image_left_out(ctx, layout, device):
    """equal output sizes and dst_offsets[i] = i * frame_stride: a [n, H, W, 3] / [n, 3, H, W] tensor; the frame of the image that
    is not in the list keeps the fill"""
    ks = [4, 5, 6, 7, 8]
    W, H = 24, 16
    frame = 3 * W * H
    s_off, _, s_len = place([SET[k][:2] for k in ks], layout, "tight", "8")
    src = np.zeros(s_len, np.uint8)
    for i, k in enumerate(ks):
        view(src, s_off[i], 0, SET[k][0], SET[k][1], layout)[...] = as_layout(source(k), layout)
    dst = np.full(len(ks) * frame, FILL, np.uint8)
    listed = [0, 1, 3, 4]
    run(ctx, device, src, dst, [s_off[i] for i in listed], [SET[ks[i]][0] for i in listed], [SET[ks[i]][1] for i in listed],
        [i * frame for i in listed], [W] * 4, [H] * 4, filter="bilinear", layout=layout)
    tensor = dst.reshape((len(ks), 3, H, W) if layout == "planar" else (len(ks), H, W, 3))
    for i, k in enumerate(ks):
        if i in listed:
            assert np.array_equal(tensor[i], as_layout(rr.resize(source(k), W, H, "bilinear"), layout)), i
        else:
            assert (tensor[i] == FILL).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_leave_the_output_untouched(ctx, device):
    import video_coding_amd as hvc
    good = (40, 24, 20, 12)
    src = np.zeros(3 * 4200 + 3 * 40 * 24 + 64, np.uint8)
    cases = [
        (dict(filter=3), [good], None, None, -1),                                   # an unknown filter
        (dict(filter=-1), [good], None, None, -1),
        (dict(layout=2), [good], None, None, -1),
        ({}, [good, (40, 24, 0, 12)], None, None, -1),                              # a size of 0
        ({}, [good, (40, 0, 20, 12)], None, None, -1),
        ({}, [good, (40, 24, 20, -1)], None, None, -1),
        ({}, [good], [119], None, -1),                                              # a stride below the row
        ({}, [good], None, [59], -1),
        (dict(filter="box"), [good, (2049, 1, 1, 1)], None, None, -7),              # over the table bound: 2049 taps at a position
        (dict(filter="bicubic"), [good, (1, 4200, 1, 1)], None, None, -7),
    ]
    for kw, images, s_str, d_str, code in cases:
        dst = np.full(4096, FILL, np.uint8)
        with pytest.raises(hvc.HvcError) as e:
            run(ctx, device, src, dst, [0, 3 * 40 * 24][:len(images)], [i[0] for i in images], [i[1] for i in images],
                [0, 1024][:len(images)], [i[2] for i in images], [i[3] for i in images], src_row_strides=s_str, dst_row_strides=d_str, **kw)
        assert e.value.code == code, (kw, images)
        assert (dst == FILL).all(), (kw, images)
    # and the same call without the fault goes through: the context is as it was
    dst = np.full(4096, FILL, np.uint8)
    src[:3 * 40 * 24] = rc.noise(40, 24).reshape(-1)
    run(ctx, device, src, dst, [0], [40], [24], [0], [20], [12], filter="box")
    assert np.array_equal(dst[:720].reshape(12, 20, 3), rr.resize(rc.noise(40, 24), 20, 12, "box")) and (dst[720:] == FILL).all()
    # the arithmetic setting has no part in it
    ctx.set_arithmetic("libjpeg")
    dst2 = np.full(4096, FILL, np.uint8)
    run(ctx, device, src, dst2, [0], [40], [24], [0], [20], [12], filter="box")
    assert np.array_equal(dst2, dst)


def test_profiling_brackets_both_passes(ctx):
    import torch
    img = rc.noise(64, 48)
    d_src, d_dst = torch.from_numpy(img.reshape(-1)).cuda(), torch.zeros(3 * 24 * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.set_profiling(True)
    ctx.rgb_resize_mixed(d_src, [0], [64], [48], d_dst, [0], [24], [16], filter="bicubic")
    ctx.synchronize()
    assert ctx.last_kernel_ms() > 0
    assert np.array_equal(d_dst.cpu().numpy().reshape(16, 24, 3), rr.resize(img, 24, 16, "bicubic"))
