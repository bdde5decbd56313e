"""Mixed batches to RGB on the GPU: hvc_yuv_to_rgb_mixed (one launch of k_ycc_to_rgb_mixed over images of any size and
sampling), hvc_decode_frames_mixed_rgb and hvc_jpeg_decode_batch_mixed_rgb.  The expected bytes come from the numpy
definition (tools/rgb_reference.planes_to_rgb) and from the single-geometry entry points -- hvc_yuv_to_rgb,
hvc_decode_frames_rgb, hvc_jpeg_decode_rgb -- called on each image alone; never from the code under test."""
import os
import pathlib
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden_bytes
from helpers import jpeg_optimised_tables
from test_gpu_mixed import check_files, file_set, make_frame, run_mixed, shapes, table  # noqa: F401  (file_set, shapes: fixtures)
from test_host_entropy import unusual_sampling_file
from test_mixed_rgb_plan import CONVERTIBLE, FACTORS, UNCONVERTIBLE, make_image
from test_restart_intervals import QT, random_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rgb_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0x5A


@pytest.fixture()
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


def up(v, a):
    return -(-v // a) * a


def image_bytes(layout, w, h, stride):
    return stride * h * (3 if layout == "planar" else 1)


def view(buf, off, stride, w, h, layout):
    import video_coding_amd as hvc
    return hvc.hvc.rgb_view(buf, off, stride, w, h, layout)


def written_mask(n, items, layout):
    """the bytes of a buffer of n that the images (off, stride, w, h) cover"""
    mask = np.zeros(n, dtype=bool)
    for off, stride, w, h in items:
        if w * h:
            view(mask, off, stride, w, h, layout)[...] = True
    return mask


# ---------------------------------------------------------------------------
# the colour pass alone

def image_list():
    """(w, h, sampling): the smallest sizes at which the lane arithmetic can go wrong"""
    out = [(w, h, s) for s in (420, 422, 444, 400) for w in (1, 7, 8, 9, 15, 16, 17, 72) for h in (1, 2, 3, 14)]
    out += [(64, 16, 420), (40, 26, 420)]              # 64 and 65 lanes (72 x 14 at 4:2:0, 63 lanes, is in the cross)
    out.insert(50, (24, 0, 420))                       # no pixel, in the middle
    out += [(520, 264, 422), (8, 2056, 400)]           # more than one workgroup; one lane per row
    out += [(33, 5, 420), (33, 5, 422), (33, 5, 444), (33, 5, 400)]   # all four samplings adjacent
    return out


def edge_image_list():
    """The smallest set with, in ONE launch, a last workgroup with spare units, a unit with a single active lane and images
    with one lane per row (groups == 1): the single-block image and the 40 x 104 4:4:4 image (9 units, 8 lanes in the last),
    and two images of 65 lanes, one of them with one lane per row."""
    out = [(8, 8, 444), (40, 104, 444), (8, 65, 400), (40, 13, 444)]
    lanes = [-(-w // 8) * (-(-h // 2) if s == 420 else h) for w, h, s in out]
    assert sum(-(-n // 64) for n in lanes) % 4 != 0 and any(n % 64 == 1 for n in lanes) and any(w <= 8 for w, _, _ in out)
    return out


class Planes:
    """seeded random planes of the images, decoded-style (whole blocks, strides on 8) or raw (stride = width + 1), the
    records `align` apart, with the numpy definition's image of each"""

    def __init__(self, hvc, decoded, align, images=None):
        rng = np.random.Generator(np.random.PCG64(20261018 + decoded))
        self.images = images or image_list()
        self.infos, self.offsets, self.want = [], [], {}
        off, parts = 3 if align == 1 else 0, []
        for k, (w, h, s) in enumerate(self.images):
            info = make_image(hvc.hvc, w, h, s, pad_w=1, decoded=decoded)
            off = up(off, align)
            rec = rng.integers(0, 256, size=info.pixel_bytes, dtype=np.uint8)
            self.infos.append(info)
            self.offsets.append(off)
            parts.append((off, rec))
            off += info.pixel_bytes
            if w * h:
                pl = []
                for i in range(info.n_comp):
                    L = info.layout[i]
                    rows = (info.pixel_bytes - L.plane_offset) // L.stride
                    pl.append(rec[L.plane_offset:L.plane_offset + rows * L.stride].reshape(rows, L.stride))
                for layout in ("interleaved", "planar"):
                    self.want[k, layout] = ref.planes_to_rgb(pl[0], pl[1] if s != 400 else None, pl[2] if s != 400 else None, s, w, h, layout)
        self.yuv = np.zeros(off + 8, dtype=np.uint8)
        for o, rec in parts:
            self.yuv[o:o + rec.size] = rec
        self.alone = {}

    def image_alone(self, ctx, k, layout):
        """hvc_yuv_to_rgb on image k alone (host memory, tight rows), computed once"""
        if (k, layout) not in self.alone:
            w, h, s = self.images[k]
            info = self.infos[k]
            comps = [dict(blocks_w=info.layout[i].blocks_w, blocks_h=info.layout[i].blocks_h, qtab=0, coef_offset=0,
                          plane_offset=info.layout[i].plane_offset, stride=info.layout[i].stride) for i in range(3)]
            out = np.zeros(3 * w * h, dtype=np.uint8)
            ctx.yuv_to_rgb(np.ascontiguousarray(self.yuv[self.offsets[k]:self.offsets[k] + info.pixel_bytes]), comps, s, w, h, out, layout=layout)
            self.alone[k, layout] = out.reshape((3, h, w) if layout == "planar" else (h, w, 3))
        return self.alone[k, layout]


_PLANES = {}


def planes_of(decoded, align, edge=False):
    import video_coding_amd as hvc
    if (decoded, align, edge) not in _PLANES:
        _PLANES[decoded, align, edge] = Planes(hvc, decoded, align, edge_image_list() if edge else None)
    return _PLANES[decoded, align, edge]


def flags_by_rule(info, s, yoff, roff, stride, layout):
    """the vec_* flags by the documented rule: every row of the plane / image on 8 bytes (chroma of 4:2:0 and 4:2:2: on 4)"""
    L = info.layout
    vy = (yoff + L[0].plane_offset) % 8 == 0 and L[0].stride % 8 == 0
    ca = 8 if s == 444 else 4
    vc = s != 400 and all((yoff + L[i].plane_offset) % ca == 0 and L[i].stride % ca == 0 for i in (1, 2))
    vr = roff % 8 == 0 and stride % 8 == 0 and (layout != "planar" or (stride * info.height) % 8 == 0)
    return vy, vc, vr


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("form", ["bytes", "vector"])
def test_colour_pass_over_images_of_any_geometry(ctx, form, device, layout, reverse):
    """form bytes: raw planes at odd strides, records and images packed at align 1 (off 8 bytes: the byte paths); form vector:
    decoded planes, images at align 256 with rows on 8 (the 8-byte paths)"""
    colour_pass(ctx, form, device, layout, reverse, False, FILL, 16)


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("form", ["bytes", "vector"])
def test_colour_pass_spare_units_single_lane_one_lane_per_row(ctx, form, layout):
    """edge_image_list() in one launch, whole buffer over a 0xA5 fill with a guard region behind the last image"""
    colour_pass(ctx, form, True, layout, False, True, 0xA5, 4096)


def colour_pass(ctx, form, device, layout, reverse, edge, FILL, guard):
    import torch
    decoded, align, row_align = (False, 1, 1) if form == "bytes" else (True, 256, 8)
    P = planes_of(decoded, align, edge)
    order = list(range(len(P.images)))[::-1] if reverse else list(range(len(P.images)))
    infos = [P.infos[k] for k in order]
    yoffs = [P.offsets[k] for k in order]
    roffs, strides, off = [], [], 5 if align == 1 else 0
    for k in order:
        w, h, s = P.images[k]
        off = up(off, align)
        stride = up(w * (1 if layout == "planar" else 3), row_align)
        roffs.append(off)
        strides.append(stride)
        off += image_bytes(layout, w, h, stride)
    rgb = np.full(off + guard, FILL, dtype=np.uint8)
    give_strides = None if row_align == 1 else strides          # (NULL = tight rows)
    if device:
        d_y, d_r = torch.from_numpy(P.yuv).cuda(), torch.from_numpy(rgb).cuda()
        assert d_y.data_ptr() % 8 == 0 and d_r.data_ptr() % 8 == 0
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.yuv_to_rgb_mixed(d_y, yoffs, infos, d_r, roffs, give_strides, layout)
        ctx.synchronize()
        ctx.reset_stream()
        rgb = d_r.cpu().numpy()
    else:
        ctx.yuv_to_rgb_mixed(P.yuv, yoffs, infos, rgb, roffs, give_strides, layout)
    mask = written_mask(rgb.size, [(roffs[j], strides[j]) + P.images[k][:2] for j, k in enumerate(order)], layout)
    assert (rgb[~mask] == FILL).all()                           # between rows, between records, behind the last one
    seen = {}
    for j, k in enumerate(order):
        w, h, s = P.images[k]
        if w * h == 0:
            continue
        got = view(rgb, roffs[j], strides[j], w, h, layout)
        assert np.array_equal(got, P.want[k, layout]), (k, P.images[k])                  # the definition
        assert np.array_equal(got, P.image_alone(ctx, k, layout)), (k, P.images[k])      # hvc_yuv_to_rgb on it alone
        seen.setdefault(s, set()).add(flags_by_rule(P.infos[k], s, yoffs[j], roffs[j], strides[j], layout))
    for s in () if edge else (420, 422, 444, 400):              # each path ran for each sampling
        want = form == "vector"
        assert any(f[0] == want for f in seen[s]) and any(f[2] == want for f in seen[s]), (s, seen[s])
        if s != 400:
            assert any(f[1] == want for f in seen[s]), (s, seen[s])


def test_colour_pass_refusals_and_an_empty_set(ctx):
    import video_coding_amd as hvc
    P = planes_of(True, 256)
    rgb = np.full(4096, FILL, dtype=np.uint8)
    ctx.yuv_to_rgb_mixed(P.yuv, [], [], rgb, [])
    ctx.yuv_to_rgb_mixed(P.yuv, [0], [make_image(hvc.hvc, 24, 0, 420)], rgb, [0])
    bad = make_image(hvc.hvc, 16, 8, 444)
    bad.comp[0].hscale = 4                                      # 4:1:1
    for args in (([0], [bad], rgb, [0], None, "interleaved"), ([0], [P.infos[0]], rgb, [0], None, 2),
                 ([0], [P.infos[40]], rgb, [0], [3], "interleaved")):
        with pytest.raises(hvc.HvcError) as e:
            ctx.yuv_to_rgb_mixed(P.yuv, *args)
        assert e.value.code == -1
    assert (rgb == FILL).all()


def test_profiling_brackets_the_colour_kernel(ctx):
    import torch
    P = planes_of(True, 256)
    k = P.images.index((520, 264, 422))
    d_y, d_r = torch.from_numpy(P.yuv).cuda(), torch.zeros(3 * 520 * 264, dtype=torch.uint8, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_profiling(True)
    try:
        ctx.yuv_to_rgb_mixed(d_y, [P.offsets[k]], [P.infos[k]], d_r, [0])
        ctx.synchronize()
        ms = ctx.last_kernel_ms()
    finally:
        ctx.set_profiling(False)
        ctx.reset_stream()
    assert 0 < ms < 50
    assert np.array_equal(d_r.cpu().numpy().reshape(264, 520, 3), P.want[k, "interleaved"])


# ---------------------------------------------------------------------------
# records to RGB

def as_image(fr, w, h, sampling):
    """a frame of test_gpu_mixed.make_frame as a w x h image of that sampling"""
    info = fr["info"]
    info.width, info.height = w, h
    for i, (hs, vs) in enumerate(FACTORS[sampling] if sampling else []):
        info.comp[i].hscale, info.comp[i].vscale = hs, vs
    return dict(fr, w=w, h=h, sampling=sampling)


def frame_alone_rgb(ctx, fr, layout):
    """hvc_decode_frames_rgb on that frame alone (host memory)"""
    specs = [dict(blocks_w=bw, blocks_h=bh, qtab=qt, coef_offset=fr["info"].layout[i].coef_offset, plane_offset=0, stride=bw * 8)
             for i, (bw, bh, qt) in enumerate(fr["planes"])]
    out = np.zeros((3, fr["h"], fr["w"]) if layout == "planar" else (fr["h"], fr["w"], 3), dtype=np.uint8)
    ctx.decode_frames_rgb(fr["coefs"], fr["info"].coef_count, np.stack(fr["tables"]), specs, fr["sampling"], 1, fr["w"], fr["h"], out,
                          layout=layout)
    return out


def run_mixed_rgb(ctx, frames, device, layout, align=64, row_align=1):
    import torch
    co, ro, strides, c, r = [], [], [], 0, 0
    for fr in frames:
        co.append(c)
        c += fr["coefs"].size
        r = up(r, align)
        ro.append(r)
        strides.append(up(fr["w"] * (1 if layout == "planar" else 3), row_align))
        r += image_bytes(layout, fr["w"], fr["h"], strides[-1])
    coefs = np.concatenate([fr["coefs"] for fr in frames] + [np.zeros(64, np.int16)])
    rgb = np.full(r + 8, FILL, dtype=np.uint8)
    infos = [fr["info"] for fr in frames]
    if device:
        d_c, d_r = torch.from_numpy(coefs).cuda(), torch.from_numpy(rgb).cuda()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.decode_frames_mixed_rgb(d_c, co, infos, d_r, ro, strides, layout)
        ctx.synchronize()
        ctx.reset_stream()
        rgb = d_r.cpu().numpy()
    else:
        ctx.decode_frames_mixed_rgb(coefs, co, infos, rgb, ro, strides, layout)
    return rgb, ro, strides


def check_frames_rgb(ctx, frames, rgb, ro, strides, layout):
    mask = written_mask(rgb.size, [(ro[j], strides[j], fr["w"], fr["h"]) for j, fr in enumerate(frames)], layout)
    assert (rgb[~mask] == FILL).all()
    for j, fr in enumerate(frames):
        if fr["w"] * fr["h"]:
            assert np.array_equal(view(rgb, ro[j], strides[j], fr["w"], fr["h"], layout), frame_alone_rgb(ctx, fr, layout)), j


@pytest.fixture(scope="module")
def rgb_shapes(shapes):  # noqa: F811
    """the shape list of test_gpu_mixed as images with odd sizes inside their decoded planes; the frame with an empty component
    has no image (width 0) and is still decoded"""
    sizes = [(8, 8, 400), (61, 63, 420), (70, 64, 444), (8, 2056, 400), (517, 263, 422), (0, 0, 0)]
    return [as_image(dict(fr, info=type(fr["info"]).from_buffer_copy(fr["info"])), *s) for fr, s in zip(shapes, sizes)]


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_records_to_rgb(ctx, rgb_shapes, device, layout):
    rgb, ro, strides = run_mixed_rgb(ctx, rgb_shapes, device, layout, row_align=8 if device else 1)
    check_frames_rgb(ctx, rgb_shapes, rgb, ro, strides, layout)
    assert ctx.last_wide_blocks() == 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_records_to_rgb_with_different_tables(ctx, device):
    """the table mix of test_gpu_mixed (qualities 20, 75, 95, a 16-bit table) on three-component frames; every block through the
    int64 arithmetic gives the same images; hvc_last_wide_blocks counts as after hvc_decode_frames_mixed"""
    q16 = table(0, 50).copy()
    q16[5] = 300
    planes = [(7, 5, 0), (4, 3, 1), (4, 3, 1)]
    frames = [make_frame(planes, [table(0, q), table(1, q)], 100 + q) for q in (20, 75, 95)]
    frames.insert(2, make_frame(planes, [q16, table(1, 20)], 300))
    frames.append(make_frame(planes, [table(0, 20), table(1, 20)], 400))
    frames = [as_image(fr, 55, 39, 420) for fr in frames]
    run_mixed(ctx, frames, device)
    wide_yuv = ctx.last_wide_blocks()
    assert wide_yuv == 35
    rgb, ro, strides = run_mixed_rgb(ctx, frames, device, "interleaved")
    assert ctx.last_wide_blocks() == wide_yuv
    check_frames_rgb(ctx, frames, rgb, ro, strides, "interleaved")
    ctx.set_decode_kernel(2)
    try:
        run_mixed(ctx, frames, device)
        wide_all = ctx.last_wide_blocks()
        again, _, _ = run_mixed_rgb(ctx, frames, device, "interleaved")
        assert ctx.last_wide_blocks() == wide_all == 5 * (35 + 12 + 12)
    finally:
        ctx.set_decode_kernel(0)
    assert np.array_equal(again, rgb)


# ---------------------------------------------------------------------------
# files to RGB

@pytest.fixture(scope="module")
def rgb_files():
    files, kinds = [golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")], [420, 420]
    for (w, h) in ((40, 24), (97, 51)):
        for k, s in enumerate(CONVERTIBLE + UNCONVERTIBLE):
            files.append(unusual_sampling_file(s, w, h, 1000 + 10 * k + w)[0])
            kinds.append((420, 422, 444, 400, 400, 0, 0, 0)[k])
    for s in (422, 444, 400):
        assert kinds.count(s) >= 2
    assert kinds.count(420) >= 2 and kinds.count(0) >= 2
    return files, kinds


_ALONE = {}


def file_alone(ctx, data, layout):
    """hvc_jpeg_decode_rgb of that file, computed once per layout and setting"""
    key = (data, layout)
    if key not in _ALONE:
        _ALONE[key] = ctx.jpeg_decode_rgb(data, layout)[1]
    return _ALONE[key]


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("threads", [1, 3])
def test_files_to_rgb(ctx, rgb_files, threads, device, layout):
    files, kinds = rgb_files
    results = ctx.jpeg_decode_batch_mixed_rgb(files, threads=threads, chunk_bytes=40000, device=device, layout=layout,
                                              row_align=8 if threads == 3 else 0)
    assert ctx.last_batch_stats.chunks >= 5 and ctx.last_batch_stats.threads == threads
    for f, (data, kind, (status, info, image)) in enumerate(zip(files, kinds, results)):
        if kind == 0:
            assert status == -1 and image is None, f
            continue
        assert status == 0, f
        image = image.cpu().numpy() if hasattr(image, "cpu") else image
        assert np.array_equal(image, file_alone(ctx, data, layout)), f


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_failing_file_stops_nobody_else(ctx, rgb_files, device):
    import torch
    import video_coding_amd as hvc
    files, kinds = rgb_files
    files, kinds = list(files), list(kinds)
    info = hvc.hvc.jpeg_read_header(files[1])
    cut = files[1][:info.ecs_offset + 2000] + b"\xff\x00" * 64 + b"\xff\xd9"   # (as in test_gpu_mixed: one-bits follow the cut)
    with pytest.raises(hvc.HvcError) as e:
        hvc.hvc.jpeg_entropy_decode(cut)
    cut_code = e.value.code
    garbage = np.random.Generator(np.random.PCG64(3)).integers(0, 256, size=3000, dtype=np.uint8).tobytes()
    rec = np.zeros(3 * 64 * 64, dtype=np.int64).reshape(3, 64, 64)
    rec[0, :, 0] = 2047 * (np.arange(64) + 1)                                  # absolute DCs beyond int16
    wide_dc = jpeg_optimised_tables(64, 64, 444, np.stack([table(0, 75), table(1, 75)]), rec.reshape(-1), table_sets=2)
    bad = {3: (cut, cut_code), 9: (garbage, None), 14: (wide_dc, -5)}
    for at in sorted(bad):
        files.insert(at, bad[at][0])
        kinds.insert(at, -1)
    lay = hvc.hvc.jpeg_mixed_rgb_layout(files, "interleaved", 64, 8)
    assert lay.status[9] != 0 and lay.status[3] == 0 and lay.status[14] == 0
    rgb = np.full(lay.total_bytes, 0xA5, dtype=np.uint8)
    if device:
        rgb = torch.from_numpy(rgb).cuda()
    results = ctx.jpeg_decode_batch_mixed_rgb(files, threads=2, chunk_bytes=60000, device=device, rgb_layout=lay, rgb=rgb)   # HVC_OK
    assert results[3][0] == cut_code != 0 and results[14][0] == -5 and results[9][0] == lay.status[9]
    assert all(results[at][2] is None for at in bad)
    host = rgb.cpu().numpy() if device else rgb
    for at in (3, 14):                                                         # their records keep the sentinel
        i, off = lay.infos[at], lay.rgb_offsets[at]
        assert (host[off:off + lay.rgb_row_strides[at] * i.height] == 0xA5).all(), at
    for f, (data, kind, (status, _, image)) in enumerate(zip(files, kinds, results)):
        if kind > 0:
            image = image.cpu().numpy() if hasattr(image, "cpu") else image
            assert status == 0 and np.array_equal(image, file_alone(ctx, data, "interleaved")), f
        elif kind == 0:
            assert status == -1
    good = rgb_files[0][:5]                                                    # and the context decodes another batch
    for data, (status, _, image) in zip(good, ctx.jpeg_decode_batch_mixed_rgb(good, threads=2, device=device)):
        image = image.cpu().numpy() if hasattr(image, "cpu") else image
        assert status == 0 and np.array_equal(image, file_alone(ctx, data, "interleaved"))


def test_settings_and_arguments(ctx, rgb_files):
    import ctypes as C
    import video_coding_amd as hvc
    files = rgb_files[0][:4]
    lay = hvc.hvc.jpeg_mixed_rgb_layout(files)
    rgb = np.full(lay.total_bytes, 0x11, dtype=np.uint8)
    ctx.set_arithmetic("hardcaml")
    try:
        with pytest.raises(hvc.HvcError) as e:
            ctx.jpeg_decode_batch_mixed_rgb(files, rgb_layout=lay, rgb=rgb)
        assert e.value.code == -1
        P = planes_of(True, 256)
        for call in (lambda: ctx.yuv_to_rgb_mixed(P.yuv, [0], [P.infos[0]], rgb, [0]),
                     lambda: ctx.decode_frames_mixed_rgb(np.zeros(64, np.int16), [0], [P.infos[0]], rgb, [0])):
            with pytest.raises(hvc.HvcError) as e:
                call()
            assert e.value.code == -1
    finally:
        ctx.set_arithmetic("model")
    assert (rgb == 0x11).all()
    L, n, st = hvc.lib(), len(files), hvc.hvc.BatchStats()

    def call(offsets=lay.rgb_offsets, cap=rgb.size, layout=0, where=0):
        status = (C.c_int * n)(*lay.status)
        return L.hvc_jpeg_decode_batch_mixed_rgb(ctx._h, lay.ptrs, lay.sizes, n, 2, 0, lay.infos, status, offsets, lay.rgb_row_strides,
                                                 rgb.ctypes.data, cap, layout, where, C.byref(st))
    assert call(cap=lay.total_bytes - 1) == -1                                 # rgb_cap too small
    beyond = (C.c_size_t * n)(*lay.rgb_offsets)
    beyond[2] = lay.total_bytes + 1
    assert call(offsets=beyond) == -1                                          # an offset beyond the cap
    assert call(layout=2) == -1 and call(where=2) == -1
    assert (rgb == 0x11).all()
    assert call() == 0 and not (rgb == 0x11).all()


def test_restart_markers(ctx):
    """one file with DRI, hvc_set_restart_markers on and off, against hvc_jpeg_decode_rgb under the same setting (the files of
    test_gpu_mixed: the model's reading of the first stays inside int16)"""
    rec, _ = random_record([(2, 2), (1, 1), (1, 1)], 200, 72, 9)
    blocks = rec.reshape(-1, 64).copy()
    rng = np.random.Generator(np.random.PCG64(1))
    blocks[:, 0] = 40
    blocks[rng.integers(0, len(blocks), size=30), 0] = rng.integers(-200, 200, size=30)
    blocks[rng.random(len(blocks)) < 0.6, 1:] = 0
    marked = jpeg_optimised_tables(200, 72, 420, QT, blocks.reshape(-1), restart_interval=5)
    files = [golden_bytes("mini.jpg"), marked]
    images = {}
    for honour in (False, True):
        ctx.set_restart_markers(honour)
        try:
            results = ctx.jpeg_decode_batch_mixed_rgb(files, threads=2)
            assert [r[0] for r in results] == [0, 0]
            for f, (_, _, image) in zip(files, results):
                assert np.array_equal(image, ctx.jpeg_decode_rgb(f)[1])        # the same setting, one file at a time
            images[honour] = results[1][2].copy()
        finally:
            ctx.set_restart_markers(False)
    assert not np.array_equal(images[False], images[True])


# ---------------------------------------------------------------------------
# the YUV path and the command line

def test_the_yuv_path_is_unchanged(ctx, file_set):  # noqa: F811
    import video_coding_amd as hvc
    files, models = file_set
    chunk = 40000
    coef_bytes = [2 * hvc.hvc.jpeg_read_header(f).coef_count for f in files]
    chunks, cur, cnt, largest = 0, 0, 0, 0                                      # the chunking rule, restated
    for b in coef_bytes:
        if chunks == 0 or (cnt > 0 and cur + b > chunk):
            chunks, cur, cnt = chunks + 1, 0, 0
        cur, cnt = cur + b, cnt + 1
        largest = max(largest, cnt)
    for device in (False, True):
        results = ctx.jpeg_decode_batch_mixed(files, threads=2, chunk_bytes=chunk, device=device)
        check_files(results, models)
        st = ctx.last_batch_stats
        assert (st.chunks, st.frames_per_chunk, st.coef_bytes) == (chunks, largest, sum(coef_bytes))


def test_cli_decode_frames_rgb(tmp_path, capsys):
    from video_coding_amd.__main__ import main
    golden = pathlib.Path(GOLDEN)
    third = tmp_path / "third.jpg"
    third.write_bytes(unusual_sampling_file(FACTORS[422], 97, 51, 4)[0])
    odd = tmp_path / "odd.jpg"
    odd.write_bytes(unusual_sampling_file(UNCONVERTIBLE[0], 40, 24, 5)[0])
    ins = [golden / "mini.jpg", golden / "Mouse480.jpg", third]
    out = tmp_path / "out"
    main(["model", "decode", "frames", str(out)] + [str(p) for p in ins] + ["-rgb"])
    for p in ins:
        one = tmp_path / (p.stem + "_one.ppm")
        main(["model", "decode", "frame", str(p), str(one), "-rgb"])
        assert (out / (p.stem + ".ppm")).read_bytes() == one.read_bytes(), p
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        main(["model", "decode", "frames", str(tmp_path / "out2"), str(ins[0]), str(odd), "-rgb"])
    assert e.value.code == 1 and "odd.jpg" in capsys.readouterr().err
    assert (tmp_path / "out2" / "mini.ppm").read_bytes() == (out / "mini.ppm").read_bytes()
    main(["model", "decode", "frames", str(tmp_path / "out3")] + [str(p) for p in ins])      # without -rgb: the .yuv files as before
    for p in ins:
        one = tmp_path / (p.stem + "_one.yuv")
        main(["model", "decode", "frame", str(p), str(one)])
        assert (tmp_path / "out3" / (p.stem + ".yuv")).read_bytes() == one.read_bytes(), p
