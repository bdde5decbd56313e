"""hvc_set_mixed_arithmetic(HVC_ARITH_LIBJPEG) on the GPU (include/hvc_jpeg.h, "Bit-exact to libjpeg"; csrc/hvc_mixed_libjpeg.hip):
k_islow_mixed and k_ycc_to_rgb_fancy_mixed through the mixed decode calls against the numpy definition
(tools/libjpeg_reference.py, tools/resize_reference.py), against the single-file calls of a second context under
hvc_set_arithmetic(HVC_ARITH_LIBJPEG), and against the stored hashes of Pillow's own output (tests/golden/libjpeg_pins.json,
libjpeg_resized_pins.json).  Every comparison is exact equality; output buffers are filled with 0xA5 and compared whole, so
padding, the gaps between records and refused outputs must keep their fill (one documented exception, host output of the file
pipelines: `whole` below).  The shapes are the smallest at which the kernels
can go wrong, not the workload's."""
import json
import os
import pathlib
import sys

import numpy as np
import pytest

import libjpeg_files as lf
from conftest import GOLDEN, golden_bytes
from test_gpu_libjpeg import extreme_record, guard_record
from test_gpu_mixed_rgb import edge_image_list, image_list, up, view
from test_host_entropy import unusual_sampling_file
from test_mixed_rgb_plan import UNCONVERTIBLE, make_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import libjpeg_reference as lj  # noqa: E402
import make_libjpeg_resized_pins as mk  # noqa: E402
import resize_reference as rr  # noqa: E402
from jpeg_opt_writer import jpeg_optimised_tables  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
E_INVALID_ARG, E_RANGE = -1, -5


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture()
def ctx(hvc):
    """the context under test: the mixed setting is libjpeg, hvc_set_arithmetic stays at its default"""
    c = hvc.Context(0)
    c.set_mixed_arithmetic("libjpeg")
    yield c
    c.close()


@pytest.fixture(scope="module")
def single(hvc):
    """a second context: the per-file calls under hvc_set_arithmetic(HVC_ARITH_LIBJPEG)"""
    c = hvc.Context(0)
    c.set_arithmetic("libjpeg")
    yield c
    c.close()


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


# ---- the setting ------------------------------------------------------------------------------------------------------
def small_frames():
    return [frame([(9, 7, 0), (3, 1, 1), (3, 1, 1)], ordinary_tables(5), 50), frame([(1, 1, 0)], ordinary_tables(6)[:1], 51)]


def test_the_setting(hvc):
    Err = hvc.hvc.HvcError
    a, b = hvc.Context(0), hvc.Context(0)
    try:
        assert a.mixed_arithmetic == "model" and b.mixed_arithmetic == "model"      # the default
        a.set_mixed_arithmetic("libjpeg")
        assert a.mixed_arithmetic == "libjpeg" and b.mixed_arithmetic == "model"    # per context
        assert a.arithmetic == "model"                                              # and no part of hvc_set_arithmetic
        for bad in ("hardcaml", 2, 7):
            with pytest.raises(Err) as e:
                a.set_mixed_arithmetic(bad)
            assert e.value.code == E_INVALID_ARG and a.mixed_arithmetic == "libjpeg"
        frames = small_frames()
        lib_bytes, _ = run_planes(a, frames, False, "tight")
        assert np.array_equal(lib_bytes, want_planes(frames, "tight")[0])
        model_bytes, _ = run_planes(b, frames, False, "tight")
        assert not np.array_equal(model_bytes, lib_bytes)
        a.set_mixed_arithmetic("model")                                             # back: the model call's bytes again
        assert a.mixed_arithmetic == "model"
        assert np.array_equal(run_planes(a, frames, False, "tight")[0], model_bytes)
        # the mixed setting governs: hvc_set_arithmetic is not looked at
        a.set_mixed_arithmetic("libjpeg")
        a.set_arithmetic("hardcaml")
        assert np.array_equal(run_planes(a, frames, False, "tight")[0], lib_bytes)
        a.set_mixed_arithmetic("model")                                             # ... and at the default it is, as before
        with pytest.raises(Err) as e:
            run_planes(a, frames, False, "tight")
        assert e.value.code == E_INVALID_ARG
    finally:
        a.close()
        b.close()


# ---- records to planes ------------------------------------------------------------------------------------------------
def ordinary_tables(seed, n=2):
    return list(np.random.default_rng(seed).integers(1, 13, size=(n, 64)).astype(np.uint16))


def frame(planes, tables, seed, coefs=None):
    """planes: (blocks_w, blocks_h, table index) each; tables: arrays of 64; the tight coefficient record is seeded: sparse small
    coefficients, every block inside the guard (or `coefs`, per plane)"""
    rng = np.random.default_rng(seed)
    rec = []
    for i, (bw, bh, t) in enumerate(planes):
        if coefs is not None:
            c = np.asarray(coefs[i]).reshape(bw * bh, 64)
        else:
            c = rng.integers(-30, 31, size=(bw * bh, 64)) * (rng.random(size=(bw * bh, 64)) < 0.3)
            c[:, 0] = rng.integers(-80, 81, size=bw * bh)
        rec.append(c.astype(np.int16).reshape(-1))
    return dict(planes=planes, tables=[np.asarray(t, dtype=np.uint16) for t in tables], coefs=np.concatenate(rec))


def info_of(hvc, fr, place):
    """the frame's JpegInfo with its planes placed tight, or spread: a stride beyond the row, room in front of and between planes"""
    info = hvc.hvc.JpegInfo()
    info.n_comp, info.n_qtabs = len(fr["planes"]), len(fr["tables"])
    for t, q in enumerate(fr["tables"]):
        for k in range(64):
            info.qtabs[t][k] = int(q[k])
    co, po = 0, 0 if place == "tight" else 16
    for i, (bw, bh, qt) in enumerate(fr["planes"]):
        L = info.layout[i]
        L.blocks_w, L.blocks_h, L.qtab, L.coef_offset, L.plane_offset = bw, bh, qt, co, po
        L.stride = bw * 8 + (0 if place == "tight" else 8)
        co += bw * bh * 64
        po += L.stride * bh * 8 + (0 if place == "tight" else 24)
    info.coef_count, info.pixel_bytes = co, po
    return info


def lay_out(hvc, frames, place):
    infos = [info_of(hvc, fr, place) for fr in frames]
    co, po, c, p = [], [], 0, 0
    for fr, info in zip(frames, infos):
        co.append(c)
        po.append(p)
        c += fr["coefs"].size
        p += up(info.pixel_bytes, 256 if place == "tight" else 64) + (0 if place == "tight" else 8)
    return infos, co, po, p + 8


def want_planes(frames, place):
    """(the whole output buffer by the definition, the blocks outside the guard)"""
    import video_coding_amd
    infos, co, po, total = lay_out(video_coding_amd, frames, place)
    out = np.full(total, FILL, dtype=np.uint8)
    wide = 0
    for fr, info, off in zip(frames, infos, po):
        at = 0
        for i, (bw, bh, t) in enumerate(fr["planes"]):
            blk = fr["coefs"][at:at + bw * bh * 64].reshape(bh, bw, 64)
            at += bw * bh * 64
            wide += int(np.count_nonzero(~lj.takes_int32_path(blk, fr["tables"][t])))
            L = info.layout[i]
            rows = off + L.plane_offset + np.arange(bh * 8)[:, None] * L.stride + np.arange(bw * 8)[None, :]
            out[rows] = lj.islow_plane(blk, fr["tables"][t], bw, bh)
    return out, wide


def run_planes(ctx, frames, device, place):
    """hvc_decode_frames_mixed into a buffer of FILL -> (the whole buffer, hvc_last_wide_blocks)"""
    import torch
    import video_coding_amd
    infos, co, po, total = lay_out(video_coding_amd, frames, place)
    coefs = np.concatenate([fr["coefs"] for fr in frames] + [np.zeros(64, np.int16)])
    pixels = np.full(total, FILL, dtype=np.uint8)
    if device:
        d_c, d_p = torch.from_numpy(coefs).cuda(), torch.from_numpy(pixels).cuda()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ctx.decode_frames_mixed(d_c, co, infos, d_p, po)
            ctx.synchronize()
        finally:
            ctx.reset_stream()
        pixels = d_p.cpu().numpy()
    else:
        ctx.decode_frames_mixed(coefs, co, infos, pixels, po)
    return pixels, ctx.last_wide_blocks()


_SHAPES = {}


def shape_frames():
    """first planes of 1, 63, 64, 65, 255, 256 and 257 blocks, a 1 x 257 plane (bw == 1, magic 0); one- and three-component
    frames; two tables per frame, some shared between frames and some distinct"""
    if not _SHAPES:
        qa, qb, qc, qd, qe = ordinary_tables(1, 5)
        _SHAPES["all"] = [
            frame([(1, 1, 0)], [qa], 11),
            frame([(9, 7, 0), (3, 1, 1), (3, 1, 1)], [qa, qb], 12),
            frame([(8, 8, 0), (4, 2, 1), (4, 2, 1)], [qc, qb], 13),
            frame([(13, 5, 0), (2, 2, 1), (2, 2, 1)], [qa, qd], 14),
            frame([(51, 5, 1)], [qa, qb], 15),
            frame([(16, 16, 0), (8, 8, 1), (8, 8, 1)], [qe, qa], 16),
            frame([(257, 1, 0)], [qc], 17),
            frame([(1, 257, 1)], [qb, qd], 18),
        ]
        assert [f["planes"][0][0] * f["planes"][0][1] for f in _SHAPES["all"]] == [1, 63, 64, 65, 255, 256, 257, 257]
    return _SHAPES["all"]


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("place", ["tight", "spread"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_records_to_planes(ctx, device, place, reverse):
    frames = shape_frames()[::-1] if reverse else shape_frames()
    want, wide = want_planes(frames, place)
    got, got_wide = run_planes(ctx, frames, device, place)
    assert np.array_equal(got, want)
    assert wide == 0 and got_wide == 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("units", [1, 3, 4, 5])
def test_sets_whose_last_workgroup_has_spare_units(ctx, units, device):
    s = shape_frames()
    frames = {1: [s[0]], 3: [s[1]], 4: [s[0], s[1]], 5: [s[4], s[0]]}[units]
    assert sum(-(-bw * bh // 64) for fr in frames for bw, bh, _ in fr["planes"]) == units
    want, _ = want_planes(frames, "tight")
    got, got_wide = run_planes(ctx, frames, device, "tight")
    assert np.array_equal(got, want) and got_wide == 0


def extreme_frames():
    """tables of all 65535, of random 16-bit entries and of 255 under random int16 coefficients, dense and sparse, lone DCs at
    +-32767 and -32768 (extreme_record); blocks with the guard sum exactly HVC_IS_GUARD_SUM and one above it in the same
    wavefront as ordinary blocks (guard_record); an ordinary frame between them"""
    out = []
    for q, planes, coefs in (extreme_record(), guard_record()):
        parts, at = [], 0
        for bw, bh, _ in planes:
            parts.append(coefs.reshape(-1)[at:at + bw * bh * 64])
            at += bw * bh * 64
        out.append(frame(planes, list(q), 0, coefs=parts))
    out.insert(1, shape_frames()[1])
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_extremes_and_both_sides_of_the_guard(ctx, device):
    frames = extreme_frames()
    want, wide = want_planes(frames, "spread")
    assert wide > 100
    got, got_wide = run_planes(ctx, frames, device, "spread")
    assert np.array_equal(got, want)
    assert got_wide == wide                               # == (~takes_int32_path).sum()
    ctx.set_decode_kernel(2)                              # every block down the int64 path: identical bytes
    try:
        again, _ = run_planes(ctx, frames, device, "spread")
    finally:
        ctx.set_decode_kernel(0)
    assert np.array_equal(again, want)


def test_profiling_brackets_the_block_kernel(ctx):
    ctx.set_profiling(True)
    try:
        got, _ = run_planes(ctx, shape_frames(), True, "tight")
        ms = ctx.last_kernel_ms()
    finally:
        ctx.set_profiling(False)
    assert 0 < ms < 50
    assert np.array_equal(got, want_planes(shape_frames(), "tight")[0])


# ---- the colour pass alone --------------------------------------------------------------------------------------------
def fancy_image_list():
    """image_list() of tests/test_gpu_mixed_rgb.py (with its (24, 0, 420) entry, an image with no pixel, and (520, 264, 422): a lane
    row longer than a wavefront, so horizontal neighbours lie in another unit) plus what the triangle filter adds"""
    out = image_list()
    assert (24, 0, 420) in out and (520, 264, 422) in out
    out += [(w, 3, s) for s in (420, 422) for w in range(1, 7)]   # cw <= 2 replicates, cw = 3 filters
    out += [(9, h, 420) for h in range(1, 5)]                     # ch = 1, 2: both vertical neighbours clamp
    out += [(24, 70, 420)]                                        # a unit spanning many rows: vertical neighbours in another unit
    return out


class Planes:
    """seeded random planes of the images, decoded-style (whole blocks, strides on 8) or raw (stride = width + 1), the records
    `align` apart, with the numpy definition's image of each (as the class of that name in tests/test_gpu_mixed_rgb.py)"""

    def __init__(self, hvc, decoded, align, images=None):
        rng = np.random.Generator(np.random.PCG64(20261020 + decoded))
        self.images = images or fancy_image_list()
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
                    self.want[k, layout] = lj.planes_to_rgb(pl[0], pl[1] if s != 400 else None, pl[2] if s != 400 else None, s, w, h, layout)
        self.yuv = np.zeros(off + 8, dtype=np.uint8)
        for o, rec in parts:
            self.yuv[o:o + rec.size] = rec


_PLANES = {}


def planes_of(decoded, align, edge=False):
    import video_coding_amd
    if (decoded, align, edge) not in _PLANES:
        _PLANES[decoded, align, edge] = Planes(video_coding_amd, decoded, align, edge_image_list() if edge else None)
    return _PLANES[decoded, align, edge]


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("form", ["bytes", "vector"])
def test_colour_pass_with_fancy_upsampling(ctx, form, device, layout, reverse):
    """form bytes: raw planes at odd strides, records and images packed at align 1 (the byte paths); form vector: decoded planes,
    images at align 256 with rows on 8 (the 8-byte paths)"""
    fancy_colour_pass(ctx, form, device, layout, reverse, False, 16)


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("form", ["bytes", "vector"])
def test_fancy_colour_pass_spare_units_single_lane_one_lane_per_row(ctx, form, layout):
    """edge_image_list() of tests/test_gpu_mixed_rgb.py in one launch: spare units in the last workgroup, a unit with a single
    active lane, images with one lane per row; whole buffer over the fill with a guard region behind the last image"""
    fancy_colour_pass(ctx, form, True, layout, False, True, 4096)


def fancy_colour_pass(ctx, form, device, layout, reverse, edge, guard):
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
        off += stride * h * (3 if layout == "planar" else 1)
    rgb = np.full(off + guard, FILL, dtype=np.uint8)
    expect = rgb.copy()
    for j, k in enumerate(order):
        w, h, s = P.images[k]
        if w * h:
            view(expect, roffs[j], strides[j], w, h, layout)[...] = P.want[k, layout]
    give_strides = None if row_align == 1 else strides          # (NULL = tight rows)
    if device:
        d_y, d_r = torch.from_numpy(P.yuv).cuda(), torch.from_numpy(rgb).cuda()
        assert d_y.data_ptr() % 8 == 0 and d_r.data_ptr() % 8 == 0
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ctx.yuv_to_rgb_mixed(d_y, yoffs, infos, d_r, roffs, give_strides, layout)
            ctx.synchronize()
        finally:
            ctx.reset_stream()
        rgb = d_r.cpu().numpy()
    else:
        ctx.yuv_to_rgb_mixed(P.yuv, yoffs, infos, rgb, roffs, give_strides, layout)
    bad = [P.images[k] for j, k in enumerate(order) if P.images[k][0] * P.images[k][1]
           and not np.array_equal(view(rgb, roffs[j], strides[j], P.images[k][0], P.images[k][1], layout), P.want[k, layout])]
    assert bad == []
    assert np.array_equal(rgb, expect)                          # between rows, between records, behind the last one: the fill


# ---- records to RGB ---------------------------------------------------------------------------------------------------
def rgb_frames():
    """(frame, w, h, sampling): images with odd sizes inside their decoded planes, different tables per frame"""
    q = ordinary_tables(9, 6)
    return [(frame([(7, 5, 0), (4, 3, 1), (4, 3, 1)], [q[0], q[1]], 31), 55, 39, 420),
            (frame([(9, 8, 0), (9, 8, 1), (9, 8, 1)], [q[2], q[3]], 32), 70, 64, 444),
            (frame([(1, 1, 0)], [q[4]], 33), 5, 3, 400),
            (frame([(66, 4, 0), (33, 4, 1), (33, 4, 1)], [q[5], q[0]], 34), 517, 29, 422),
            (frame([(2, 2, 0), (1, 1, 1), (1, 1, 1)], [q[1], q[2]], 35), 4, 9, 420)]


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_records_to_rgb(ctx, hvc, device, layout):
    import torch
    items = rgb_frames()
    infos, co, ro, strides, c, r = [], [], [], [], 0, 0
    for fr, w, h, s in items:
        info = info_of(hvc, fr, "tight")
        info.width, info.height = w, h
        for i, (hs, vs) in enumerate(lf.FACTORS[s]):
            info.comp[i].hscale, info.comp[i].vscale = hs, vs
        infos.append(info)
        co.append(c)
        c += fr["coefs"].size
        r = up(r, 64)
        ro.append(r)
        strides.append(up(w * (1 if layout == "planar" else 3), 8 if device else 1))
        r += strides[-1] * h * (3 if layout == "planar" else 1)
    coefs = np.concatenate([fr["coefs"] for fr, _, _, _ in items] + [np.zeros(64, np.int16)])
    rgb = np.full(r + 8, FILL, dtype=np.uint8)
    expect = rgb.copy()
    for j, (fr, w, h, s) in enumerate(items):
        view(expect, ro[j], strides[j], w, h, layout)[...] = lj.record_to_rgb(fr["coefs"], np.stack(fr["tables"]), fr["planes"], s, w, h, layout)
    if device:
        d_c, d_r = torch.from_numpy(coefs).cuda(), torch.from_numpy(rgb).cuda()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        try:
            ctx.decode_frames_mixed_rgb(d_c, co, infos, d_r, ro, strides, layout)
            ctx.synchronize()
        finally:
            ctx.reset_stream()
        rgb = d_r.cpu().numpy()
    else:
        ctx.decode_frames_mixed_rgb(coefs, co, infos, rgb, ro, strides, layout)
    assert np.array_equal(rgb, expect)
    assert ctx.last_wide_blocks() == 0


# ---- files ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(ROOT, "tests", "golden", "libjpeg_pins.json")) as f:
        return json.load(f)["rgb_sha256"]


@pytest.fixture(scope="module")
def resized_pins():
    with open(os.path.join(ROOT, "tests", "golden", "libjpeg_resized_pins.json")) as f:
        return json.load(f)["rgb_sha256"]


def status_of(fn):
    import video_coding_amd
    try:
        return 0, fn()[1]
    except video_coding_amd.hvc.HvcError as e:
        return e.code, None


@pytest.fixture(scope="module")
def file_set(hvc, single):
    """every size of libjpeg_files.SIZES x the four samplings x the three FAMILIES plus the golden files, and in the middle a
    truncated file, a file with a DC beyond int16 and a 4:1:1 file -> dict(files, names (pinned ones), planes / rgb: what
    hvc_jpeg_decode / hvc_jpeg_decode_rgb of the second context give for each file alone: (status, bytes))"""
    files, names = [], []
    for fam in range(len(lf.FAMILIES)):
        for sampling in (420, 422, 444, 400):
            for w, h in lf.SIZES:
                files.append(bytes(lf.writer_file(lf.seed_of(w, h, sampling, fam), w, h, sampling, lf.FAMILIES[fam])[0]))
                names.append(lf.pin_name(w, h, sampling, fam, 0) if (w, h, sampling, fam, 0) in lf.PINNED else None)
    for name in lf.GOLDEN_FILES:
        files.append(golden_bytes(name))
        names.append(name)
    mouse = golden_bytes("Mouse480.jpg")
    cut = mouse[:hvc.hvc.jpeg_read_header(mouse).ecs_offset + 2000] + b"\xff\x00" * 64 + b"\xff\xd9"   # (one-bits follow the cut)
    dc = np.array([[20000] + [0] * 63, [40000] + [0] * 63], dtype=np.int64)                              # absolute DC 60000
    wide_dc = bytes(jpeg_optimised_tables(16, 8, [(1, 1)], np.ones((2, 64), dtype=np.uint16), dc))
    odd = bytes(unusual_sampling_file(UNCONVERTIBLE[0], 45, 53, 77)[0])                                  # 4:1:1
    for at, data in ((40, cut), (41, wide_dc), (80, odd)):
        files.insert(at, data)
        names.insert(at, None)
    planes = [status_of(lambda d=d: single.jpeg_decode(d)) for d in files]
    rgb = {layout: [status_of(lambda d=d: single.jpeg_decode_rgb(d, layout)) for d in files] for layout in ("interleaved", "planar")}
    assert planes[40][0] not in (0, E_RANGE) and planes[41][0] == E_RANGE and planes[80][0] == 0
    assert rgb["interleaved"][41][0] == E_RANGE and rgb["interleaved"][80][0] == E_INVALID_ARG
    assert sum(n is not None for n in names) == len(lf.PINNED) - 1 + len(lf.GOLDEN_FILES)
    return dict(files=files, names=names, planes=planes, rgb=rgb)


def whole(got, expect, device, spans, taken, good):
    """the buffers compared whole.  Host output only: the alignment padding between the records of two consecutive good files is
    nobody's and, as include/hvc_jpeg.h says of hvc_jpeg_decode_batch_mixed, may be overwritten -- those bytes alone are left out;
    spans: (first byte, end) of every file's record in file order, taken: the files the layout gave a record (the others take
    no room and no part), good: the files whose status is 0"""
    keep = np.ones(got.size, dtype=bool)
    if not device:
        part = [f for f in range(len(spans)) if taken[f]]
        for a, b in zip(part, part[1:]):
            if good[a] and good[b] and spans[a][1] <= spans[b][0]:
                keep[spans[a][1]:spans[b][0]] = False
    return np.array_equal(got[keep], expect[keep])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("reader", ["host", "gpu"])
@pytest.mark.parametrize("threads", [1, 3])
def test_files_to_planes_and_to_rgb(ctx, hvc, file_set, pins, threads, reader, device):
    import torch
    files, n = file_set["files"], len(file_set["files"])
    ctx.set_mixed_reader(reader)
    # planes
    lay = hvc.hvc.jpeg_mixed_layout(files)
    pixels = np.full(lay.total_bytes + 8, FILL, dtype=np.uint8)
    expect = pixels.copy()
    for f in range(n):
        st, rec = file_set["planes"][f]
        if st == 0:
            expect[lay.pixel_offsets[f]:lay.pixel_offsets[f] + rec.size] = rec
    buf = torch.from_numpy(pixels).cuda() if device else pixels
    results = ctx.jpeg_decode_batch_mixed(files, threads=threads, chunk_bytes=40000, device=device, layout=lay, pixels=buf)
    assert ctx.last_batch_stats.chunks >= 5
    assert [r[0] for r in results] == [file_set["planes"][f][0] for f in range(n)]   # every status is the file's own
    # good files: the per-file call's bytes; everything else, the failed files' records among it: the fill
    spans = [(lay.pixel_offsets[f], lay.pixel_offsets[f] + lay.infos[f].pixel_bytes) for f in range(n)]
    assert whole(host(buf), expect, device, spans, [lay.status[f] == 0 for f in range(n)], [r[0] == 0 for r in results])
    gpu_files = ctx.last_mixed_reader_files()[0]
    assert gpu_files > 0 if reader == "gpu" else gpu_files == 0
    # RGB
    layout = "planar" if threads == 3 else "interleaved"
    rlay = hvc.hvc.jpeg_mixed_rgb_layout(files, layout, 64, 8 if device else 0)
    rgb = np.full(rlay.total_bytes + 8, FILL, dtype=np.uint8)
    expect = rgb.copy()
    for f in range(n):
        st, img = file_set["rgb"][layout][f]
        if st == 0:
            i = rlay.infos[f]
            view(expect, rlay.rgb_offsets[f], rlay.rgb_row_strides[f], i.width, i.height, layout)[...] = img
    buf = torch.from_numpy(rgb).cuda() if device else rgb
    results = ctx.jpeg_decode_batch_mixed_rgb(files, threads=threads, chunk_bytes=40000, device=device, rgb_layout=rlay, rgb=buf)
    assert [r[0] for r in results] == [file_set["rgb"][layout][f][0] for f in range(n)]
    got = host(buf)
    spans = [(rlay.rgb_offsets[f], rlay.rgb_offsets[f] + rlay.rgb_row_strides[f] * rlay.infos[f].height * (3 if layout == "planar" else 1))
             for f in range(n)]
    assert whole(got, expect, device, spans, [rlay.status[f] == 0 for f in range(n)], [r[0] == 0 for r in results])
    gpu_files = ctx.last_mixed_reader_files()[0]
    assert gpu_files > 0 if reader == "gpu" else gpu_files == 0
    for f, name in enumerate(file_set["names"]):                 # Pillow's own pixels
        if name is not None:
            i = rlay.infos[f]
            img = view(got, rlay.rgb_offsets[f], rlay.rgb_row_strides[f], i.width, i.height, layout)
            assert lf.sha256(img.transpose(1, 2, 0) if layout == "planar" else img) == pins[name], name


@pytest.mark.parametrize("reader", ["host", "gpu"])
def test_restart_intervals_honoured(ctx, hvc, single, pins, reader):
    case = (64, 48, 420, 0, 3)
    files = [golden_bytes("mini.jpg"), bytes(lf.pinned_file(case)[0]), bytes(lf.pinned_file(lf.PINNED[0])[0])]
    ctx.set_mixed_reader(reader)
    ctx.set_restart_markers(True)
    single.set_restart_markers(True)
    try:
        results = ctx.jpeg_decode_batch_mixed_rgb(files, threads=2)
        planes = ctx.jpeg_decode_batch_mixed(files, threads=2)
        assert [r[0] for r in results] == [0, 0, 0] and [r[0] for r in planes] == [0, 0, 0]
        for data, (_, _, image) in zip(files, results):
            assert np.array_equal(image, single.jpeg_decode_rgb(data)[1])
        for data, (_, info, pl) in zip(files, planes):
            rec = single.jpeg_decode(data)[1]
            for k, p in enumerate(pl):
                L = info.layout[k]
                assert np.array_equal(p, rec[L.plane_offset:L.plane_offset + p.size].reshape(p.shape)), k
    finally:
        single.set_restart_markers(False)
        ctx.set_restart_markers(False)
    assert lf.sha256(results[1][2]) == pins[lf.pin_name(*case)]
    assert lf.sha256(results[0][2]) == pins["mini.jpg"]


# ---- resized ----------------------------------------------------------------------------------------------------------
_RGB = {}


def libjpeg_image(single, data):
    if data not in _RGB:
        _RGB[data] = single.jpeg_decode_rgb(data)[1]
    return _RGB[data]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("filt", mk.FILTERS)
def test_files_to_one_resized_tensor(ctx, single, resized_pins, filt, layout, device):
    import torch
    named = mk.files()
    names, files = list(named), list(named.values())
    n, (W, H) = len(files), (24, 16)
    ctx.set_restart_markers(True)                                # (one of the pinned files carries restart intervals)
    single.set_restart_markers(True)
    try:
        out = np.full(n * 3 * W * H + 16, FILL, dtype=np.uint8)
        expect = out.copy()
        for f, data in enumerate(files):
            img = rr.resize(libjpeg_image(single, data), W, H, filt)
            expect[f * 3 * W * H:(f + 1) * 3 * W * H] = (img.transpose(2, 0, 1) if layout == "planar" else img).reshape(-1)
        buf = torch.from_numpy(out).cuda() if device else out
        status, tensor = ctx.jpeg_decode_batch_mixed_resized(files, size=(W, H), filter=filt, layout=layout, device=device, threads=2,
                                                             chunk_bytes=40000, out=buf)
    finally:
        single.set_restart_markers(False)
        ctx.set_restart_markers(False)
    assert status == [0] * n
    got = host(buf)
    assert np.array_equal(got, expect)
    for f, name in enumerate(names):                             # Pillow's Image.open(f).convert("RGB").resize((W, H), filter)
        img = got[f * 3 * W * H:(f + 1) * 3 * W * H].reshape((3, H, W) if layout == "planar" else (H, W, 3))
        assert lf.sha256(img.transpose(1, 2, 0) if layout == "planar" else img) == resized_pins[mk.pin_key(name, W, H, filt)], name


def test_a_size_per_file(ctx, single, resized_pins):
    named = mk.files()
    names, files = list(named), list(named.values())
    sizes = [mk.SIZES[f % len(mk.SIZES)] for f in range(len(files))]
    ctx.set_restart_markers(True)
    single.set_restart_markers(True)
    try:
        status, views = ctx.jpeg_decode_batch_mixed_resized(files, sizes=sizes, filter="bicubic", threads=2)
        want = [rr.resize(libjpeg_image(single, data), w, h, "bicubic") for data, (w, h) in zip(files, sizes)]
    finally:
        single.set_restart_markers(False)
        ctx.set_restart_markers(False)
    assert status == [0] * len(files)
    for f, (name, (w, h)) in enumerate(zip(names, sizes)):
        assert np.array_equal(views[f], want[f]), name
        assert lf.sha256(views[f]) == resized_pins[mk.pin_key(name, w, h, "bicubic")], name


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_scaled_forms_refuse_with_their_output_untouched(ctx, hvc, single):
    Err = hvc.hvc.HvcError
    files = [golden_bytes("mini.jpg"), bytes(lf.pinned_file(lf.PINNED[0])[0])]
    out = np.full(1 << 16, FILL, dtype=np.uint8)

    def refused(fn):
        with pytest.raises(Err) as e:
            fn()
        assert e.value.code == E_INVALID_ARG
        assert (out == FILL).all()

    info = hvc.hvc.jpeg_read_header(files[0])
    _, coefs = hvc.hvc.jpeg_entropy_decode(files[0])
    sinfo = hvc.hvc.jpeg_scaled_info(info, 2)
    refused(lambda: ctx.decode_frames_mixed_scaled(coefs, [0], [sinfo], 2, out, [0]))
    refused(lambda: ctx.jpeg_decode_batch_mixed_scaled(files, 2, pixels=out))
    refused(lambda: ctx.jpeg_decode_batch_mixed_scaled_rgb(files, 2, rgb=out))
    refused(lambda: ctx.jpeg_decode_batch_mixed_resized(files, size=(24, 16), scale_denom=2, out=out))
    # the next full-size call on the same context succeeds
    results = ctx.jpeg_decode_batch_mixed_rgb(files, threads=2)
    assert [r[0] for r in results] == [0, 0]
    for data, (_, _, image) in zip(files, results):
        assert np.array_equal(image, single.jpeg_decode_rgb(data)[1])


# ---- the command line -------------------------------------------------------------------------------------------------
def test_cli_decode_frames_arithmetic_libjpeg(tmp_path):
    from video_coding_amd.__main__ import main
    golden = pathlib.Path(GOLDEN)
    third = tmp_path / "third.jpg"
    third.write_bytes(bytes(lf.pinned_file(lf.PINNED[1])[0]))
    ins = [golden / "mini.jpg", golden / "Mouse480.jpg", third]
    out = tmp_path / "out"
    main(["model", "decode", "frames", str(out)] + [str(p) for p in ins] + ["-rgb", "-arithmetic", "libjpeg"])
    for p in ins:
        one = tmp_path / (p.stem + "_one.ppm")
        main(["model", "decode", "frame", str(p), str(one), "-rgb", "-arithmetic", "libjpeg"])
        assert (out / (p.stem + ".ppm")).read_bytes() == one.read_bytes(), p
    model = tmp_path / "model"
    main(["model", "decode", "frames", str(model)] + [str(p) for p in ins] + ["-rgb"])
    assert (model / "mini.ppm").read_bytes() != (out / "mini.ppm").read_bytes()
