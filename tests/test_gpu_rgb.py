"""RGB on the GPU (include/hvc_jpeg.h, RGB; csrc/hvc_rgb.hip): k_ycc_to_rgb / k_rgb_to_ycc and the entry points built on
them against the numpy definition (tools/rgb_reference.py, which tests/test_rgb_reference.py holds to libjpeg and to the
checker's resampling) composed with the checker's block stage.  Every comparison is exact equality."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

from conftest import golden_bytes
from helpers import synth_pixels
from oracle import orc
from test_gpu_yuv444 import geometry420, make_record, tables
from test_host_entropy import unusual_sampling_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rgb_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ("interleaved", "planar")
SAMPLINGS = (420, 422, 444, 400)
SIZES = [(1, 1), (2, 2), (3, 3), (17, 9), (18, 10), (52, 44), (53, 45), (100, 30), (1040, 32), (1042, 70), (1920, 1080),
         (1921, 1081)]
E_INVALID_ARG = -1


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture(scope="module")
def ctx(hvc):
    c = hvc.Context(0)
    yield c
    c.close()


def up(x, a):
    return (x + a - 1) // a * a


def plane_record(sampling, w, h, pad=True):
    """(specs, bytes per frame, [(offset, stride, valid w, valid h)]) of a record of three planes the way a decoder leaves
    them: pad = planes rounded up to whole MCUs (strides multiples of 8), else tight raw planes"""
    cw, ch = ref.chroma_window(sampling, w, h)
    dims = [(w, h)] + ([] if sampling == 400 else [(cw, ch), (cw, ch)])
    specs, where, off = [], [], 0
    for k, (pw, ph) in enumerate(dims):
        sw, sh = (up(pw, 16 if k == 0 else 8), up(ph, 16 if k == 0 else 8)) if pad else (pw, ph)
        specs.append(dict(blocks_w=0, blocks_h=0, plane_offset=off, stride=sw))
        where.append((off, sw, sh))
        off += sw * sh
    return specs, up(off, 8) if pad else off, where


def random_planes(seed, n, sampling, w, h, pad=True):
    """n frames of random planes (the whole record is random: what lies outside the windows must not matter)"""
    specs, fs, where = plane_record(sampling, w, h, pad)
    rng = np.random.Generator(np.random.PCG64(seed))
    rec = rng.integers(0, 256, size=(n, fs), dtype=np.uint8)
    planes = [[rec[f, o:o + sw * sh].reshape(sh, sw) for (o, sw, sh) in where] for f in range(n)]
    return specs, fs, rec, planes


def want_rgb(planes, sampling, w, h, layout):
    p = list(planes) + [None, None]
    return ref.planes_to_rgb(p[0], p[1], p[2], sampling, w, h, layout)


def to_rgb(ctx, hvc, rec, specs, fs, sampling, w, h, layout, device, row_stride=0, frame_stride=0, fill=0xA5):
    """hvc_yuv_to_rgb on n frames -> the whole output buffer as uint8 [n, frame bytes]"""
    import torch
    n = rec.shape[0]
    tight = 3 * w * h
    rs = row_stride or (w if layout == "planar" else 3 * w)
    fb = frame_stride or rs * (3 * h if layout == "planar" else h)
    out = np.full((n, fb), fill, dtype=np.uint8)
    assert fb >= tight
    if device:
        d_in, d_out = torch.from_numpy(rec).cuda(), torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        ctx.yuv_to_rgb(d_in, specs, sampling, w, h, d_out, n_frames=n, yuv_frame_stride=fs, layout=layout, rgb_row_stride=row_stride,
                       rgb_frame_stride=frame_stride)
        ctx.synchronize()
        return d_out.cpu().numpy()
    ctx.yuv_to_rgb(rec, specs, sampling, w, h, out, n_frames=n, yuv_frame_stride=fs, layout=layout, rgb_row_stride=row_stride,
                   rgb_frame_stride=frame_stride)
    return out


def image_of(buf, w, h, layout, row_stride=0):
    """the image inside one frame's buffer, and a mask of the bytes that belong to it"""
    rs = row_stride or (w if layout == "planar" else 3 * w)
    rows = 3 * h if layout == "planar" else h
    row_bytes = w if layout == "planar" else 3 * w
    mask = np.zeros(buf.size, dtype=bool)
    mask[:rows * rs].reshape(rows, rs)[:, :row_bytes] = True
    img = buf[:rows * rs].reshape(rows, rs)[:, :row_bytes]
    return (img.reshape(3, h, w) if layout == "planar" else img.reshape(h, w, 3)), mask


# ---- colour, exhaustively
def all_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    return [((v >> s) & 255).astype(np.uint8).reshape(4096, 4096) for s in (16, 8, 0)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_ycc_triple(ctx, hvc, layout):
    y, cb, cr = all_triples()
    rec = np.concatenate([p.reshape(-1) for p in (y, cb, cr)])[None, :]
    specs = [dict(blocks_w=0, blocks_h=0, plane_offset=k << 24, stride=4096) for k in range(3)]
    got = to_rgb(ctx, hvc, rec, specs, rec.shape[1], 444, 4096, 4096, layout, True)[0]
    want = ref.planes_to_rgb(y, cb, cr, 444, 4096, 4096, layout)
    assert np.array_equal(got.reshape(want.shape), want)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_rgb_triple(ctx, hvc, layout):
    import torch
    r, g, b = all_triples()
    image = np.stack([r, g, b], axis=0 if layout == "planar" else 2)
    specs = [dict(blocks_w=0, blocks_h=0, plane_offset=k << 24, stride=4096) for k in range(3)]
    d_rgb = torch.from_numpy(np.ascontiguousarray(image)).cuda()
    d_yuv = torch.zeros(3 << 24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.rgb_to_yuv(d_rgb, 4096, 4096, 444, d_yuv, specs, layout=layout)
    ctx.synchronize()
    got = d_yuv.cpu().numpy().reshape(3, 4096, 4096)
    for k, want in enumerate(ref.rgb_to_planes(image, 444, layout)):
        assert np.array_equal(got[k], want), k


# ---- geometry
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_yuv_to_rgb_geometry(ctx, hvc, sampling, w, h):
    """two frames of decoder-shaped records (planes of whole MCUs, the odd sizes reading the ceil window), both layouts,
    device and host memory"""
    specs, fs, rec, planes = random_planes(sampling * 7 + w + h, 2, sampling, w, h)
    for layout in LAYOUTS:
        want = [want_rgb(planes[f], sampling, w, h, layout).reshape(-1) for f in range(2)]
        for device in (True, False):
            got = to_rgb(ctx, hvc, rec, specs, fs, sampling, w, h, layout, device)
            for f in range(2):
                assert np.array_equal(got[f], want[f]), (layout, device, f, int(np.flatnonzero(got[f] != want[f])[0]))


def encoder_refuses(sampling, w, h):
    return (sampling in (420, 422) and w % 2 == 1) or (sampling == 420 and h % 2 == 1)


def to_yuv(ctx, image, w, h, sampling, layout, device, pad, fill=0xA5, row_stride=0, frame_stride=0):
    """hvc_rgb_to_yuv on n images (uint8 [n, frame bytes]) -> (the whole output buffer [n, fs], where the planes are)"""
    import torch
    n = image.shape[0]
    cw, ch = (w if sampling == 444 else w // 2), (h // 2 if sampling == 420 else h)
    dims = [(w, h)] + ([] if sampling == 400 else [(cw, ch), (cw, ch)])
    specs, where, off = [], [], 0
    for (pw, ph) in dims:
        stride = up(pw, 8) + (8 if pad else 0) if pad is not None else pw
        specs.append(dict(blocks_w=0, blocks_h=0, plane_offset=off, stride=stride))
        where.append((off, stride, pw, ph))
        off += stride * ph + (3 if pad else 0)
    fs = up(off, 8) if pad is not None else off
    out = np.full((n, fs), fill, dtype=np.uint8)
    if device:
        d_in, d_out = torch.from_numpy(np.ascontiguousarray(image)).cuda(), torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        ctx.rgb_to_yuv(d_in, w, h, sampling, d_out, specs, n_frames=n, yuv_frame_stride=fs, layout=layout, rgb_row_stride=row_stride,
                       rgb_frame_stride=frame_stride)
        ctx.synchronize()
        out = d_out.cpu().numpy()
    else:
        ctx.rgb_to_yuv(np.ascontiguousarray(image), w, h, sampling, out, specs, n_frames=n, yuv_frame_stride=fs, layout=layout,
                       rgb_row_stride=row_stride, rgb_frame_stride=frame_stride)
    return out, where


def check_planes(out, where, want, fill=0xA5):
    """every plane equals `want`, every other byte of the frame's buffer is still `fill`"""
    mask = np.zeros(out.size, dtype=bool)
    for (o, stride, pw, ph), p in zip(where, want):
        idx = (o + np.arange(ph)[:, None] * stride + np.arange(pw)[None, :]).reshape(-1)
        assert np.array_equal(out[idx].reshape(ph, pw), p)
        mask[idx] = True
    assert (out[~mask] == fill).all()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_rgb_to_yuv_geometry(ctx, hvc, sampling, w, h):
    rng = np.random.Generator(np.random.PCG64(sampling * 11 + w + h))
    for layout in LAYOUTS:
        images = rng.integers(0, 256, size=(2,) + hvc.hvc.rgb_shape(layout, w, h), dtype=np.uint8)
        for device in (True, False):
            if encoder_refuses(sampling, w, h):
                with pytest.raises(hvc.hvc.HvcError) as e:
                    to_yuv(ctx, images.reshape(2, -1), w, h, sampling, layout, device, None)
                assert e.value.code == E_INVALID_ARG
                continue
            for pad in (None, False):  # tight raw planes; planes with strides of whole 8 bytes (the encoder's record)
                out, where = to_yuv(ctx, images.reshape(2, -1), w, h, sampling, layout, device, pad)
                for f in range(2):
                    want = [p for p in ref.rgb_to_planes(images[f], sampling, layout) if p is not None]
                    check_planes(out[f], where, want)


# ---- strides
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_row_and_frame_padding_is_untouched(ctx, hvc, sampling, layout):
    for (w, h, extra_row, extra_frame) in ((64, 32, 8, 64), (64, 32, 5, 13), (50, 22, 3, 7), (1040, 16, 16, 0)):
        row_bytes = w if layout == "planar" else 3 * w
        rows = 3 * h if layout == "planar" else h
        rs, fb = row_bytes + extra_row, (row_bytes + extra_row) * rows + extra_frame
        specs, fs, rec, planes = random_planes(w + extra_row, 2, sampling, w, h)
        for device in (True, False):
            got = to_rgb(ctx, hvc, rec, specs, fs, sampling, w, h, layout, device, row_stride=rs, frame_stride=fb)
            for f in range(2):
                img, mask = image_of(got[f], w, h, layout, rs)
                assert np.array_equal(img, want_rgb(planes[f], sampling, w, h, layout)), (w, device, f)
                assert (got[f][~mask] == 0xA5).all(), (w, device, f)
            # the way back: strided images in, planes with padded strides out
            rng = np.random.Generator(np.random.PCG64(w))
            buf = rng.integers(0, 256, size=(2, fb), dtype=np.uint8)
            out, where = to_yuv(ctx, buf, w, h, sampling, layout, device, True, row_stride=rs, frame_stride=fb)
            for f in range(2):
                img, _ = image_of(buf[f], w, h, layout, rs)
                check_planes(out[f], where, [p for p in ref.rgb_to_planes(img, sampling, layout) if p is not None])


def test_arguments(ctx, hvc):
    L = hvc.lib()
    specs, fs, rec, _ = random_planes(1, 1, 420, 18, 10)
    comps = hvc.hvc.components(specs)
    out = np.full(3 * 18 * 10, 0xA5, dtype=np.uint8)
    call = lambda **k: L.hvc_yuv_to_rgb(ctx._h, rec.ctypes.data, fs, comps, k.get("s", 420), k.get("w", 18), k.get("h", 10), k.get("cw", 9),
                                        k.get("ch", 5), k.get("n", 1), out.ctypes.data, k.get("rs", 0), k.get("fs", 0), k.get("layout", 0), 0)
    for bad in (dict(cw=8), dict(ch=4), dict(s=411), dict(layout=2), dict(rs=53), dict(fs=100), dict(w=-1), dict(n=-1), dict(cw=64)):
        assert call(**bad) == E_INVALID_ARG, bad
        assert (out == 0xA5).all(), bad
    for nothing in (dict(w=0), dict(h=0), dict(n=0)):
        assert call(**nothing) == 0, nothing
        assert (out == 0xA5).all(), nothing
    assert call() == 0 and not (out == 0xA5).all()
    # hvc_yuv_frame_bytes / hvc_yuv_convert keep refusing luma only
    n = C.c_size_t()
    assert L.hvc_yuv_frame_bytes(400, 16, 16, C.byref(n)) == E_INVALID_ARG


# ---- coefficient records -> RGB
def record_planes(rec, planes, qtabs):
    out, off = [], 0
    for (bw, bh, qt) in planes:
        n = bw * bh * 64
        out.append(orc.dequant_idct_recon(rec[off:off + n], qtabs[qt], bw, bh).reshape(bh * 8, bw * 8))
        off += n
    return out


def geometry(sampling, w, h):
    if sampling == 420:
        return geometry420(w, h)
    if sampling == 422:
        rw, rh = up(w, 16), up(h, 8)
        return [(rw // 8, rh // 8, 0), (rw // 16, rh // 8, 1), (rw // 16, rh // 8, 1)]
    rw, rh = up(w, 8), up(h, 8)
    return [(rw // 8, rh // 8, 0)] + ([] if sampling == 400 else [(rw // 8, rh // 8, 1)] * 2)


def decode_rgb(ctx, hvc, recs, planes, qt, sampling, w, h, layout, device):
    import torch
    specs, cfs, _ = hvc.hvc.frame_layout(planes)
    n, coefs = len(recs), np.stack(recs)
    out = np.full((n,) + hvc.hvc.rgb_shape(layout, w, h), 0xA5, dtype=np.uint8)
    if device:
        d_c, d_o = torch.from_numpy(coefs).cuda(), torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        ctx.decode_frames_rgb(d_c, cfs, qt, specs, sampling, n, w, h, d_o, layout=layout)
        ctx.synchronize()
        return d_o.cpu().numpy()
    ctx.decode_frames_rgb(coefs, cfs, qt, specs, sampling, n, w, h, out, layout=layout)
    return out


@pytest.mark.parametrize("sampling,w,h", [(420, 64, 48), (420, 53, 45), (420, 1042, 70), (420, 1056, 144), (422, 100, 30), (422, 53, 45),
                                          (444, 52, 44), (444, 17, 9), (400, 53, 45)])
def test_decode_frames_rgb_with_adversarial_blocks(ctx, hvc, sampling, w, h):
    planes, qt = geometry(sampling, w, h), tables(90)
    recs = [make_record(31 + f, planes, qt, adversarial=0.07) for f in range(2)]
    for layout in LAYOUTS:
        for device in (True, False):
            got = decode_rgb(ctx, hvc, recs, planes, qt, sampling, w, h, layout, device)
            assert ctx.last_wide_blocks() > 0
            for f, rec in enumerate(recs):
                assert np.array_equal(got[f], want_rgb(record_planes(rec, planes, qt), sampling, w, h, layout)), (layout, device, f)


@pytest.mark.parametrize("w,h", [(64, 48), (1056, 144), (52, 44)])
def test_decode_frames_rgb_equals_the_colour_pass_over_the_fused_444_frame(ctx, hvc, w, h):
    import torch
    planes, qt = geometry420(w, h), tables()
    recs = [make_record(3 + f, planes, qt, adversarial=0.05) for f in range(2)]
    specs, cfs, _ = hvc.hvc.frame_layout(planes)
    d_c = torch.from_numpy(np.stack(recs)).cuda()
    d_444 = torch.zeros((2, 3 * w * h), dtype=torch.uint8, device="cuda")
    d_rgb = torch.zeros((2, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_frames_yuv444(d_c, cfs, qt, specs, 2, w, h, d_444)
    raw = [dict(blocks_w=0, blocks_h=0, plane_offset=k * w * h, stride=w) for k in range(3)]
    ctx.yuv_to_rgb(d_444, raw, 444, w, h, d_rgb, n_frames=2, yuv_frame_stride=3 * w * h)
    ctx.synchronize()
    got = decode_rgb(ctx, hvc, recs, planes, qt, 420, w, h, "interleaved", True)
    assert np.array_equal(got, d_rgb.cpu().numpy())


def test_decode_frames_rgb_under_the_hardcaml_arithmetic(ctx, hvc):
    w, h = 100, 44
    planes, qt = geometry420(w, h), tables(60)
    recs = [make_record(50 + f, planes, qt) for f in range(2)]
    specs, cfs, pfs = hvc.hvc.frame_layout(planes)
    model = decode_rgb(ctx, hvc, recs, planes, qt, 420, w, h, "interleaved", False)
    ctx.set_arithmetic("hardcaml")
    try:
        pixels = np.zeros((2, pfs), dtype=np.uint8)
        ctx.decode_frames(np.stack(recs), cfs, qt, specs, 2, pixels, pfs)
        want = np.zeros((2, h, w, 3), dtype=np.uint8)
        ctx.yuv_to_rgb(pixels, specs, 420, w, h, want, n_frames=2, yuv_frame_stride=pfs)
        got = decode_rgb(ctx, hvc, recs, planes, qt, 420, w, h, "interleaved", False)
        got_dev = decode_rgb(ctx, hvc, recs, planes, qt, 420, w, h, "interleaved", True)
    finally:
        ctx.set_arithmetic("model")
    assert np.array_equal(got, want) and np.array_equal(got_dev, want)
    assert not np.array_equal(got, model)  # (the RTL's pixels, not the model's)
    for f in range(2):  # and `want` is the definition over those planes
        pl = [pixels[f, s["plane_offset"]:s["plane_offset"] + s["blocks_w"] * s["blocks_h"] * 64].reshape(-1, s["blocks_w"] * 8) for s in specs]
        assert np.array_equal(want[f], want_rgb(pl, 420, w, h, "interleaved"))


# ---- files
def definition_of_file(jpg, layout="interleaved"):
    d = orc.Decoder(jpg)
    d.decode()
    info = [d.info(i) for i in range(d.ncomp)]
    if d.ncomp == 1:
        sampling = 400
    else:
        hs, vs = info[0]["decoded_width"] // info[1]["decoded_width"], info[0]["decoded_height"] // info[1]["decoded_height"]
        sampling = {(2, 2): 420, (2, 1): 422, (1, 1): 444}[(hs, vs)]
    w, h = np.asarray(d.cropped_plane(0)).shape[::-1]
    return want_rgb([d.plane(i) for i in range(d.ncomp)], sampling, w, h, layout)


def frame_planes(seed, w, h, chroma):
    cw, ch = (w if chroma == 444 else w // 2), (h // 2 if chroma == 420 else h)
    big = lambda s, pw, ph: synth_pixels(s, up(ph, 8), up(pw, 8))[:ph, :pw]
    return np.ascontiguousarray(big(seed, w, h)), np.ascontiguousarray(big(seed + 1, cw, ch)), np.ascontiguousarray(big(seed + 2, cw, ch))


@pytest.mark.parametrize("name", ["Mouse480.jpg", "mini.jpg"])
def test_reference_files(ctx, hvc, name):
    jpg = golden_bytes(name)
    for layout in LAYOUTS:
        info, got = ctx.jpeg_decode_rgb(jpg, layout)
        assert got.shape == hvc.hvc.rgb_shape(layout, info.width, info.height)
        assert np.array_equal(got, definition_of_file(jpg, layout))


@pytest.mark.parametrize("w,h", [(64, 48), (53, 45), (200, 121), (643, 361)])
@pytest.mark.parametrize("chroma", [420, 422, 444])
def test_encoded_files_plain_optimised_and_with_restart_intervals(hvc, chroma, w, h):
    """files of this library's encoder (odd sizes: the encoder takes the integer halves as chroma planes, the file's chroma
    planes still hold the ceil window), with the default tables, optimised ones, and restart intervals honoured -- the
    restart file carries the plain file's record, so its image is the plain file's"""
    y, u, v = frame_planes(w + chroma, w, h, chroma)
    c = hvc.Context(0)
    try:
        plain = c.jpeg_encode(y, u, v, w, h, chroma, 80)
        want = definition_of_file(plain)
        assert want.shape == (h, w, 3)
        assert np.array_equal(c.jpeg_decode_rgb(plain)[1], want)
        c.set_huffman_tables("optimised")
        opt = c.jpeg_encode(y, u, v, w, h, chroma, 80)
        assert opt != plain and np.array_equal(c.jpeg_decode_rgb(opt, "planar")[1], want.transpose(2, 0, 1))
        c.set_restart_interval(3)
        rst = c.jpeg_encode(y, u, v, w, h, chroma, 80)
        c.set_restart_markers(True)
        assert np.array_equal(c.jpeg_decode_rgb(rst)[1], want)
        c.set_restart_markers(False)  # the model's reading (the first interval only, or an error): hvc_jpeg_decode's
        try:
            info, pixels = c.jpeg_decode(rst)
        except hvc.hvc.HvcError as e:
            with pytest.raises(hvc.hvc.HvcError) as e2:
                c.jpeg_decode_rgb(rst)
            assert e2.value.code == e.code
        else:
            assert np.array_equal(c.jpeg_decode_rgb(rst)[1], want_rgb(info.planes(pixels), chroma, w, h, "interleaved"))
    finally:
        c.close()


def test_large_file_takes_the_gpu_reader(ctx, hvc):
    """a file above the size where the single-file path hands the Huffman reader to the GPU"""
    w, h = 1923, 1081
    rng = np.random.Generator(np.random.PCG64(5))
    y, u, v = (rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    jpg = ctx.jpeg_encode(y, u, v, w, h, 420, 90)
    assert len(jpg) > 128 * 1024
    assert np.array_equal(ctx.jpeg_decode_rgb(jpg)[1], definition_of_file(jpg))


@pytest.mark.parametrize("gpu_entropy", [False, True])
@pytest.mark.parametrize("chroma,w,h", [(420, 104, 72), (422, 53, 45), (444, 72, 40)])
def test_batch_equals_the_single_files(hvc, chroma, w, h, gpu_entropy):
    """70 files of one geometry (optimised tables and restart intervals, the markers honoured) through both pipelines, to
    host and to device memory: frame by frame the single-file results"""
    import torch
    n = 70
    c = hvc.Context(0)
    try:
        c.set_huffman_tables("optimised")
        c.set_restart_interval(4)
        jpegs = [c.jpeg_encode(*frame_planes(1000 + 3 * f, w, h, chroma), w, h, chroma, 70) for f in range(n)]
        c.set_restart_markers(True)
        for layout in LAYOUTS:
            single = np.stack([c.jpeg_decode_rgb(j, layout)[1] for j in jpegs])
            assert np.array_equal(single[0], definition_of_file(c_plain(hvc, w, h, chroma, 1000), layout))
            host = np.full(single.shape, 0xA5, dtype=np.uint8)
            st = c.jpeg_decode_batch_rgb(jpegs, host, layout, threads=3, frames_per_chunk=16, gpu_entropy=gpu_entropy)
            assert st.chunks >= 4
            assert np.array_equal(host, single)
            dev = torch.full(single.shape, 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c.jpeg_decode_batch_rgb(jpegs, dev, layout, threads=3, frames_per_chunk=16, gpu_entropy=gpu_entropy)
            c.synchronize()
            assert np.array_equal(dev.cpu().numpy(), single)
    finally:
        c.close()


def c_plain(hvc, w, h, chroma, seed):
    """the plain file (no restart interval) of that frame: what the checker can decode in full"""
    c = hvc.Context(0)
    try:
        return c.jpeg_encode(*frame_planes(seed, w, h, chroma), w, h, chroma, 70)
    finally:
        c.close()


def test_batch_with_row_and_frame_strides(ctx, hvc):
    w, h, n = 52, 44, 9
    jpegs = [ctx.jpeg_encode(*frame_planes(77 + 3 * f, w, h, 420), w, h, 420, 75) for f in range(n)]
    rs, fb = 3 * w + 4, (3 * w + 4) * h + 10
    out = np.full((n, fb), 0xA5, dtype=np.uint8)
    ctx.jpeg_decode_batch_rgb(jpegs, out, "interleaved", threads=2, frames_per_chunk=4, rgb_row_stride=rs, rgb_frame_stride=fb)
    for f in range(n):
        img, mask = image_of(out[f], w, h, "interleaved", rs)
        assert np.array_equal(img, definition_of_file(jpegs[f]))
        assert (out[f][~mask] == 0xA5).all()


@pytest.mark.parametrize("sampling", [[(4, 1), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1), (2, 2)], [(1, 2), (1, 1), (1, 1)], [(2, 1), (1, 1)]])
def test_samplings_without_an_rgb_image_are_refused(ctx, hvc, sampling):
    """4:1:1, four components, 4:4:0, two components: HVC_E_INVALID_ARG, output untouched"""
    L = hvc.lib()
    jpg, _ = unusual_sampling_file(sampling, 97, 51, 17)
    info = hvc.hvc.JpegInfo()
    out = np.full(3 * 97 * 51, 0xA5, dtype=np.uint8)
    assert L.hvc_jpeg_decode_rgb(ctx._h, jpg, len(jpg), C.byref(info), out.ctypes.data, out.size, 0, 0) == E_INVALID_ARG
    assert (out == 0xA5).all()
    for gpu_entropy in (False, True):
        with pytest.raises(hvc.hvc.HvcError) as e:
            ctx.jpeg_decode_batch_rgb([jpg, jpg], out, gpu_entropy=gpu_entropy)
        assert e.value.code == E_INVALID_ARG
        assert (out == 0xA5).all()


def test_grey_file(ctx, hvc):
    jpg, _ = unusual_sampling_file([(1, 1)], 97, 51, 3)
    want = definition_of_file(jpg)
    assert np.array_equal(want[..., 0], want[..., 1]) and np.array_equal(want[..., 0], want[..., 2])
    assert np.array_equal(ctx.jpeg_decode_rgb(jpg)[1], want)
    out = np.zeros((3, 51, 97, 3), dtype=np.uint8)
    ctx.jpeg_decode_batch_rgb([jpg] * 3, out)
    assert all(np.array_equal(out[f], want) for f in range(3))


def test_libjpegs_own_planes_give_libjpegs_rgb(ctx, hvc):
    """draft("YCbCr") planes of a 4:4:4 file through hvc_yuv_to_rgb: PIL's RGB, exactly"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.Generator(np.random.PCG64(9))
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, size=(120, 200, 3), dtype=np.uint8), "RGB").save(buf, "JPEG", quality=92, subsampling=0)
    im = Image.open(io.BytesIO(buf.getvalue()))
    im.draft("YCbCr", im.size)
    ycc = np.asarray(im)
    rgb = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    rec = np.ascontiguousarray(ycc.transpose(2, 0, 1)).reshape(1, -1)
    specs = [dict(blocks_w=0, blocks_h=0, plane_offset=k * 200 * 120, stride=200) for k in range(3)]
    got = to_rgb(ctx, hvc, rec, specs, rec.shape[1], 444, 200, 120, "interleaved", False)
    assert np.array_equal(got.reshape(120, 200, 3), rgb)


# ---- encode
@pytest.mark.parametrize("ri", [0, 16])
@pytest.mark.parametrize("tables_", ["default", "optimised"])
@pytest.mark.parametrize("chroma,w,h", [(420, 64, 48), (420, 130, 66), (422, 130, 65), (444, 53, 45), (420, 1920, 1080)])
def test_jpeg_encode_rgb_is_jpeg_encode_of_the_definitions_planes(hvc, chroma, w, h, tables_, ri):
    rng = np.random.Generator(np.random.PCG64(w + h + chroma))
    smooth = np.stack([synth_pixels(60 + k, up(h, 8), up(w, 8))[:h, :w] for k in range(3)], axis=2)
    image = np.where(rng.random((h, w, 1)) < 0.02, rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), smooth).astype(np.uint8)
    c = hvc.Context(0)
    try:
        c.set_huffman_tables(tables_)
        c.set_restart_interval(ri)
        y, u, v = ref.rgb_to_planes(image, chroma)
        want = c.jpeg_encode(y, u, v, w, h, chroma, 85)
        assert c.jpeg_encode_rgb(image, chroma, 85) == want
        assert c.jpeg_encode_rgb(np.ascontiguousarray(image.transpose(2, 0, 1)), chroma, 85, layout="planar") == want
        c.set_restart_markers(True)
        c.set_huffman_tables("default")
        c.set_restart_interval(0)
        plain = c.jpeg_encode(y, u, v, w, h, chroma, 85)
        assert np.array_equal(c.jpeg_decode_rgb(want)[1], definition_of_file(plain))
    finally:
        c.close()


def test_jpeg_encode_rgb_keeps_the_encoders_rule(ctx, hvc):
    image = np.zeros((45, 53, 3), dtype=np.uint8)
    for chroma, img in ((420, image), (422, image), (420, image[:, :52]), (400, image)):
        with pytest.raises(hvc.hvc.HvcError) as e:
            ctx.jpeg_encode_rgb(np.ascontiguousarray(img), chroma, 75)
        assert e.value.code == E_INVALID_ARG
    assert ctx.jpeg_encode_rgb(np.ascontiguousarray(image[:, :52]), 422, 75)[:2] == b"\xff\xd8"


def test_cli_round_trip(tmp_path, ctx, hvc):
    from video_coding_amd.__main__ import main
    cli = lambda *argv: main([str(a) for a in argv])
    image = np.stack([synth_pixels(90 + k, 48, 64) for k in range(3)], axis=2)
    ref.write_ppm(str(tmp_path / "in.ppm"), image)
    cli("model", "encode", "frame", tmp_path / "in.ppm", "64x48", tmp_path / "out.jpg", "-rgb", "-chroma", 444, "-quality", 90)
    jpg = (tmp_path / "out.jpg").read_bytes()
    assert jpg == ctx.jpeg_encode_rgb(image, 444, 90)
    cli("model", "decode", "frame", tmp_path / "out.jpg", tmp_path / "back.ppm", "-rgb")
    back = (tmp_path / "back.ppm").read_bytes()
    assert back == b"P6\n64 48\n255\n" + definition_of_file(jpg).tobytes()


def test_the_measured_kernels_are_the_parents(hvc):
    """csrc/hvc_rgb.hip is a translation unit of its own: the kernel id the counters and the roofline line are keyed on stays"""
    assert hvc.hvc.kernel_source_id() == hvc.hvc.kernel_build_id() == "b746d7b6f0f2"
