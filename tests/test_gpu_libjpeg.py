"""hvc_set_arithmetic(HVC_ARITH_LIBJPEG) on the GPU (include/hvc_jpeg.h, "Bit-exact to libjpeg"; csrc/hvc_libjpeg.hip):
k_islow and k_ycc_to_rgb_fancy through the C ABI against the numpy definition (tools/libjpeg_reference.py, which
tests/test_libjpeg_reference.py holds to libjpeg-turbo with 0 mismatches) and against the stored hashes of Pillow's own
output (tests/golden/libjpeg_pins.json).  Every comparison is exact equality; buffers are compared whole, so what lies
between rows, planes and frames must keep its fill."""
import json
import os
import sys

import numpy as np
import pytest

import libjpeg_files as lf
from conftest import golden_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libjpeg_reference as lj  # noqa: E402
from jpeg_opt_writer import jpeg_optimised_tables  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
TILE = 256   # HVC_TILE: blocks per workgroup
E_INVALID_ARG, E_RANGE = -1, -5
GUARD = lj.spec_constants()["HVC_IS_GUARD_SUM"]


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture(scope="module")
def ctx(hvc):
    c = hvc.Context(0)
    c.set_arithmetic("libjpeg")
    yield c
    c.close()


@pytest.fixture(scope="module")
def pins():
    with open(os.path.join(ROOT, "tests", "golden", "libjpeg_pins.json")) as f:
        return json.load(f)["rgb_sha256"]


def test_the_setting_reads_back(ctx, hvc):
    assert ctx.arithmetic == "libjpeg"
    with pytest.raises(hvc.hvc.HvcError) as e:
        ctx.set_encode_arithmetic(3)
    assert e.value.code == E_INVALID_ARG and ctx.encode_arithmetic == "model"


# ---- the block stage on records -------------------------------------------------------------------------------------
def place(planes, layout):
    """specs of the planes and the bytes from frame to frame; "spread": a non-tight stride and plane offsets"""
    specs, co, po = [], 0, 0 if layout == "tight" else 16
    for bw, bh, qt in planes:
        stride = bw * 8 + (0 if layout == "tight" else 8)
        specs.append(dict(blocks_w=bw, blocks_h=bh, qtab=qt, coef_offset=co, plane_offset=po, stride=stride))
        co += bw * bh * 64
        po += stride * bh * 8 + (0 if layout == "tight" else 24)
    return specs, po + (0 if layout == "tight" else 40)


def want_buffer(coefs, q, specs, fs):
    """(the output buffer the definition gives: FILL everywhere but in the planes, blocks outside the guard)"""
    out = np.full((coefs.shape[0], fs), FILL, dtype=np.uint8)
    wide = 0
    for f in range(coefs.shape[0]):
        for s in specs:
            bw, bh = s["blocks_w"], s["blocks_h"]
            blk = coefs[f, s["coef_offset"]:s["coef_offset"] + bw * bh * 64].reshape(bh, bw, 64)
            wide += int(np.count_nonzero(~lj.takes_int32_path(blk, q[s["qtab"]])))
            rows = np.arange(bh * 8)[:, None] * s["stride"] + s["plane_offset"] + np.arange(bw * 8)[None, :]
            out[f][rows] = lj.islow_plane(blk, q[s["qtab"]], bw, bh)
    return out, wide


def run(ctx, coefs, q, specs, fs, device):
    """hvc_decode_frames into a buffer of FILL -> (the whole buffer, hvc_last_wide_blocks)"""
    n_frames, coef_fs = coefs.shape
    out = np.full((n_frames, fs), FILL, dtype=np.uint8)
    if device:
        import torch
        d_c, d_o = torch.from_numpy(coefs).cuda(), torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        ctx.decode_frames(d_c, coef_fs, q, specs, n_frames, d_o, fs)
        ctx.synchronize()
        out = d_o.cpu().numpy()
    else:
        ctx.decode_frames(coefs, coef_fs, q, specs, n_frames, out, fs)
    return out, ctx.last_wide_blocks()


def ordinary_record(seed, planes, n_frames):
    """(two tables, coefs [n_frames][elements]): sparse small coefficients, every block inside the guard"""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 17, size=(2, 64)).astype(np.uint16)
    fs = sum(bw * bh * 64 for bw, bh, _ in planes)
    c = rng.integers(-40, 41, size=(n_frames, fs // 64, 64))
    c *= rng.random(size=c.shape) < 0.3
    c[..., 0] = rng.integers(-100, 101, size=c.shape[:2])
    return q, c.reshape(n_frames, -1).astype(np.int16)


# planes of 1, 63, 64, 65 and HVC_TILE +- 1 blocks (with a second plane and a second table beside them)
SHAPES = {"1": [(1, 1, 0)], "63": [(9, 7, 0), (3, 1, 1)], "64": [(8, 8, 0), (4, 2, 1)], "65": [(13, 5, 1), (5, 13, 0)],
          "tile-1": [(51, 5, 0), (17, 15, 1)], "tile+1": [(257, 1, 0), (1, 257, 1)]}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n_frames,layout", [(1, "tight"), (3, "spread")])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_records_equal_the_definition(ctx, shape, n_frames, layout, device):
    planes = SHAPES[shape]
    assert planes[0][0] * planes[0][1] == {"1": 1, "63": 63, "64": 64, "65": 65, "tile-1": TILE - 1, "tile+1": TILE + 1}[shape]
    q, coefs = ordinary_record(len(shape) * 10 + n_frames, planes, n_frames)
    specs, fs = place(planes, layout)
    want, wide = want_buffer(coefs, q, specs, fs)
    got, got_wide = run(ctx, coefs, q, specs, fs, device)
    assert np.array_equal(got, want)
    assert wide == 0 and got_wide == 0   # ordinary blocks: none takes the int64 path


def test_dequant_idct_recon_takes_the_setting(ctx):
    q, coefs = ordinary_record(77, [(5, 3, 0)], 1)
    out = np.zeros((24, 40), dtype=np.uint8)
    ctx.dequant_idct_recon(coefs.reshape(3, 5, 64), q[0], 5, 3, 1, out)
    assert np.array_equal(out, lj.islow_plane(coefs, q[0], 5, 3))


def extreme_record():
    """tables of 65535 and of 255 under random int16 coefficients (dense and sparse), lone DCs at the formats' ends"""
    rng = np.random.default_rng(21)
    q = np.stack([np.full(64, 65535), rng.integers(1, 65536, size=64), np.full(64, 255)]).astype(np.uint16)
    planes = [(9, 4, 0), (9, 4, 1), (9, 4, 2)]
    c = rng.integers(-32768, 32768, size=(3, 36, 64))
    c[:, 12:24] *= rng.random(size=(3, 12, 64)) < 0.1
    c[:, 24:, 1:] = 0
    c[:, 24, 0], c[:, 25, 0], c[:, 26, 0] = -32768, 32767, 1
    c[0, 27] = -32768
    c[0, 28] = 32767
    return q, planes, c.reshape(1, -1).astype(np.int16)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_extremes_of_the_formats(ctx, device):
    q, planes, coefs = extreme_record()
    specs, fs = place(planes, "tight")
    want, wide = want_buffer(coefs, q, specs, fs)
    got, got_wide = run(ctx, coefs, q, specs, fs, device)
    assert np.array_equal(got, want)
    assert got_wide == wide and wide > 80   # the int64 path, and a saturating guard sum: all of these are far outside


def guard_record():
    """one plane under a table of ones and one under a table of threes: blocks with S exactly at the guard and one step
    past it, the sum in one coefficient, in two, spread over all 64, with either sign; between them ordinary blocks"""
    rng = np.random.default_rng(9)
    q = np.stack([np.ones(64), np.full(64, 3)]).astype(np.uint16)
    planes = [(10, 4, 0), (10, 4, 1)]
    c = np.zeros((2, 40, 64), dtype=np.int64)
    for t in range(2):
        g = GUARD // int(q[t, 0])   # the largest sum of |coefficients| inside
        b = 0
        for extra in (0, 1):
            for sign in (1, -1):
                c[t, b, 0] = sign * (g + extra)
                c[t, b + 1, 63] = sign * (g + extra)
                dcv = min(8184, (g + extra) // 2)   # an ordinary file's largest DC beside one AC term
                c[t, b + 2, 0], c[t, b + 2, lj.ZF[8 * 3 + 3]] = sign * dcv, -sign * (g + extra - dcv)
                c[t, b + 3] = sign * ((g + extra) // 64) * np.where(np.arange(64) % 2, 1, -1)
                c[t, b + 3, lj.ZF[8 * 7 + 1]] += sign * ((g + extra) % 64) * (1 if lj.ZF[8 * 7 + 1] % 2 else -1)
                # the worst case of the proof's tightest bound: everything in natural row 3 / column 3
                c[t, b + 4, lj.ZF[8 * 3 + 3]] = sign * (g + extra)
                b += 5
        c[t, b:] = rng.integers(-60, 61, size=(40 - b, 64)) * (rng.random(size=(40 - b, 64)) < 0.3)
    return q, planes, c.reshape(1, -1).astype(np.int16)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_both_sides_of_the_guard(ctx, device):
    q, planes, coefs = guard_record()
    blk = coefs.reshape(2, 40, 64)
    for t in range(2):
        s = lj.guard_sum(blk[t, :20], q[t])
        assert (s[:10] <= GUARD).all() and (s[:10] > GUARD - 3).all() and (s[10:] > GUARD).all() and (s[10:] <= GUARD + 3).all()
    specs, fs = place(planes, "spread")
    want, wide = want_buffer(coefs, q, specs, fs)
    got, got_wide = run(ctx, coefs, q, specs, fs, device)
    assert np.array_equal(got, want)
    assert wide == 20 and got_wide == 20


@pytest.mark.parametrize("which", ["ordinary", "guard", "extreme"])
def test_int64_path_for_every_block_gives_identical_bytes(ctx, which):
    """hvc_set_decode_kernel(ctx, 2): the cross-check of the two paths"""
    if which == "ordinary":
        planes = SHAPES["tile+1"]
        q, coefs = ordinary_record(3, planes, 2)
    else:
        q, planes, coefs = guard_record() if which == "guard" else extreme_record()
    specs, fs = place(planes, "tight")
    want, _ = want_buffer(coefs, q, specs, fs)
    a, _ = run(ctx, coefs, q, specs, fs, True)
    ctx.set_decode_kernel(2)
    try:
        b, all_wide = run(ctx, coefs, q, specs, fs, True)
    finally:
        ctx.set_decode_kernel(0)
    assert np.array_equal(a, b) and np.array_equal(b, want)
    assert all_wide == coefs.size // 64


def file_record(hvc, data):
    info, coefs = hvc.hvc.jpeg_entropy_decode(data, restart_markers=True)
    return info, coefs


def test_natural_records_stay_on_the_int_path(ctx, hvc):
    """the coefficients of a photograph, and of white noise at quality 100: no block may leave the int path"""
    info, coefs = file_record(hvc, golden_bytes("Mouse480.jpg"))
    planes = lf.planes_of_info(info)
    specs, fs = place(planes, "tight")
    want, wide = want_buffer(coefs[None], info.qtab_array(), specs, fs)
    got, got_wide = run(ctx, coefs[None], info.qtab_array(), specs, fs, True)
    assert np.array_equal(got, want) and wide == 0 and got_wide == 0
    # white noise, 64 x 48, tables of ones: the forward DCT of uniform noise in float, rounded (what a quality-100 file holds)
    rng = np.random.default_rng(64048)
    px = rng.integers(0, 256, size=(48, 8, 8)).astype(np.float64) - 128
    k = np.arange(8)
    m = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(1 / 8), 0.5)
    d = np.rint(np.einsum("ur,brc,vc->buv", m, px, m)).astype(np.int64).reshape(48, 64)
    noise = np.zeros((48, 64), dtype=np.int16)
    noise[:, lj.ZF] = d
    q = np.ones((1, 64), dtype=np.uint16)
    s = lj.guard_sum(noise, q[0])
    assert 2000 < s.max() < GUARD   # a few thousand per block
    specs, fs = place([(8, 6, 0)], "tight")
    want, wide = want_buffer(noise.reshape(1, -1), q, specs, fs)
    got, got_wide = run(ctx, noise.reshape(1, -1), q, specs, fs, True)
    assert np.array_equal(got, want) and wide == 0 and got_wide == 0


# ---- hvc_yuv_to_rgb -------------------------------------------------------------------------------------------------
RGB_SIZES = [(1, 1), (3, 2), (4, 4), (5, 5), (6, 3), (17, 9), (18, 10), (53, 45), (64, 48)]


def up(x, a):
    return (x + a - 1) // a * a


@pytest.mark.parametrize("row_align", [0, 8], ids=["tight_rows", "rows_on_8"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("sampling", [420, 422, 444, 400])
def test_yuv_to_rgb_equals_the_definition(ctx, sampling, layout, row_align):
    """planes with junk beyond the chroma window, 2 frames a frame stride apart, every size: both store paths (rows on
    8-byte boundaries take the 8-byte stores where the planes allow it), both sides of cw <= 2, odd windows, both edge rules"""
    import torch
    rng = np.random.default_rng(sampling + len(layout) + row_align)
    for w, h in RGB_SIZES:
        cw, ch = lj.chroma_window(sampling, w, h)
        pw, ph = up(w, 16), up(h, 16)   # the planes: padded, 8-byte rows
        planes = rng.integers(0, 256, size=(2, 3, ph, pw), dtype=np.uint8)   # (junk beyond the windows included)
        specs = [dict(blocks_w=0, blocks_h=0, qtab=0, coef_offset=0, plane_offset=k * ph * pw, stride=pw) for k in range(3)]
        if sampling == 400:
            specs = specs[:1]
        row = (3 * w if layout == "interleaved" else w)
        row_stride = up(row, row_align) + row_align if row_align else 0
        rows = h if layout == "interleaved" else 3 * h
        frame_stride = (row_stride or row) * rows + (24 if row_align else 5)
        out = np.full((2, frame_stride), FILL, dtype=np.uint8)
        want = out.copy()
        for f in range(2):
            img = lj.planes_to_rgb(planes[f, 0], planes[f, 1], planes[f, 2], sampling, w, h, layout)
            at = np.arange(rows)[:, None] * (row_stride or row) + np.arange(row)[None, :]
            want[f][at] = img.reshape(rows, row)
        for device in (False, True):
            if device:
                d_y, d_o = torch.from_numpy(planes).cuda(), torch.from_numpy(out).cuda()
                torch.cuda.synchronize()
                ctx.yuv_to_rgb(d_y, specs, sampling, w, h, d_o, chroma_size=(cw, ch), n_frames=2, yuv_frame_stride=3 * ph * pw, layout=layout,
                               rgb_row_stride=row_stride, rgb_frame_stride=frame_stride)
                ctx.synchronize()
                got = d_o.cpu().numpy()
            else:
                got = out.copy()
                ctx.yuv_to_rgb(planes, specs, sampling, w, h, got, chroma_size=(cw, ch), n_frames=2, yuv_frame_stride=3 * ph * pw, layout=layout,
                               rgb_row_stride=row_stride, rgb_frame_stride=frame_stride)
            assert np.array_equal(got, want), (w, h, device)


def test_yuv_to_rgb_byte_path_of_the_planes(ctx):
    """planes at odd offsets with odd strides: the bounds-checked byte loads"""
    rng = np.random.default_rng(5)
    for sampling in (420, 422):
        w, h = 21, 11
        cw, ch = lj.chroma_window(sampling, w, h)
        buf = rng.integers(0, 256, size=3 * 40 * 37 + 3, dtype=np.uint8)
        specs = [dict(blocks_w=0, blocks_h=0, qtab=0, coef_offset=0, plane_offset=1 + k * 40 * 37, stride=37) for k in range(3)]
        p = [buf[s["plane_offset"]:s["plane_offset"] + 40 * 37].reshape(40, 37) for s in specs]
        got = np.zeros((h, w, 3), dtype=np.uint8)
        ctx.yuv_to_rgb(buf, specs, sampling, w, h, got, chroma_size=(cw, ch))
        assert np.array_equal(got, lj.planes_to_rgb(p[0], p[1], p[2], sampling, w, h))


def test_decode_frames_rgb_equals_the_definition(ctx):
    w, h, sampling = 53, 45, 420
    q, c, planes = lf.random_record(5, w, h, sampling, lf.FAMILIES[0])
    specs, _ = place(planes, "tight")
    got = np.zeros((2, h, w, 3), dtype=np.uint8)
    coefs = np.stack([c, c[::-1].reshape(-1, 64)[:, ::-1].reshape(-1)])
    ctx.decode_frames_rgb(coefs, coefs.shape[1], q, specs, sampling, 2, w, h, got)
    for f in range(2):
        assert np.array_equal(got[f], lj.record_to_rgb(coefs[f], q, planes, sampling, w, h))


# ---- files ----------------------------------------------------------------------------------------------------------
def reference_of_file(hvc, data):
    info, coefs = file_record(hvc, data)
    planes = lf.planes_of_info(info)
    return info, lj.record_planes(coefs, info.qtab_array(), planes), lj.record_to_rgb(coefs, info.qtab_array(), planes, lf.sampling_of_info(info),
                                                                                    info.width, info.height)


def padded_record(info, planes):
    out = np.zeros(info.pixel_bytes, dtype=np.uint8)
    for k, p in enumerate(planes):
        L = info.layout[k]
        rows = np.arange(p.shape[0])[:, None] * L.stride + L.plane_offset + np.arange(p.shape[1])[None, :]
        out[rows] = p
    return out


@pytest.mark.parametrize("name", lf.GOLDEN_FILES)
def test_golden_files(ctx, hvc, pins, name):
    data = golden_bytes(name)
    info, planes, rgb = reference_of_file(hvc, data)
    assert lf.sha256(rgb) == pins[name]
    _, px = ctx.jpeg_decode(data)
    assert np.array_equal(px, padded_record(info, planes))
    _, got = ctx.jpeg_decode_rgb(data)
    assert np.array_equal(got, rgb) and lf.sha256(got) == pins[name]
    _, got = ctx.jpeg_decode_rgb(data, layout="planar")
    assert np.array_equal(got, rgb.transpose(2, 0, 1))
    assert ctx.last_wide_blocks() == 0


@pytest.mark.parametrize("case", lf.PINNED, ids=lambda c: lf.pin_name(*c))
def test_writer_made_files(ctx, hvc, pins, case):
    data, q, c, planes = lf.pinned_file(case)
    ctx.set_restart_markers(bool(case[4]))
    try:
        info, ref_planes, rgb = reference_of_file(hvc, data)
        _, px = ctx.jpeg_decode(data)
        _, got = ctx.jpeg_decode_rgb(data)
    finally:
        ctx.set_restart_markers(False)
    assert np.array_equal(px, padded_record(info, ref_planes))
    assert np.array_equal(got, rgb)
    assert lf.sha256(got) == pins[lf.pin_name(*case)]


def same_geometry_files(w, h, sampling, n):
    """n files that share size, sampling and quantiser tables (a batch's rule), with different records"""
    q, _, planes = lf.random_record(900, w, h, sampling, lf.FAMILIES[0])
    files = []
    for i in range(n):
        _, c, _ = lf.random_record(901 + i, w, h, sampling, lf.FAMILIES[0])
        files.append(jpeg_optimised_tables(w, h, lf.FACTORS[sampling], q, c))
    return files


@pytest.mark.parametrize("gpu_entropy", [False, True], ids=["host_reader", "gpu_reader"])
@pytest.mark.parametrize("files", ["mini", "writer", "mouse"])
def test_batches(ctx, hvc, pins, files, gpu_entropy):
    jpegs = {"mini": [golden_bytes("mini.jpg")] * 3, "mouse": [golden_bytes("Mouse480.jpg")] * 2,
             "writer": same_geometry_files(53, 45, 420, 4)}[files]
    refs = [reference_of_file(hvc, j) for j in jpegs]
    info = refs[0][0]
    fs = up(info.pixel_bytes, 8) + 16
    out = np.full((len(jpegs), fs), FILL, dtype=np.uint8)
    ctx.jpeg_decode_batch(jpegs, out, fs, threads=2, frames_per_chunk=1, gpu_entropy=gpu_entropy)
    for f, (_, planes, _) in enumerate(refs):
        assert np.array_equal(out[f, :info.pixel_bytes], padded_record(info, planes))
        assert (out[f, info.pixel_bytes:] == FILL).all()
    rgb = np.zeros((len(jpegs), info.height, info.width, 3), dtype=np.uint8)
    ctx.jpeg_decode_batch_rgb(jpegs, rgb, threads=2, frames_per_chunk=1, gpu_entropy=gpu_entropy)
    for f, (_, _, want) in enumerate(refs):
        assert np.array_equal(rgb[f], want)
    if files != "writer":
        assert lf.sha256(rgb[0]) == pins[{"mini": "mini.jpg", "mouse": "Mouse480.jpg"}[files]]


def test_batch_to_device_memory(ctx, hvc):
    import torch
    jpegs = same_geometry_files(33, 31, 422, 3)
    refs = [reference_of_file(hvc, j) for j in jpegs]
    d_rgb = torch.zeros((3, 31, 33, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.jpeg_decode_batch_rgb(jpegs, d_rgb, threads=2, frames_per_chunk=1, gpu_entropy=True)
    ctx.synchronize()
    got = d_rgb.cpu().numpy()
    for f in range(3):
        assert np.array_equal(got[f], refs[f][2])


def test_asynchronous_submit(ctx):
    planes = SHAPES["tile-1"]
    q, coefs = ordinary_record(12, planes, 2)
    specs, fs = place(planes, "tight")
    want, _ = want_buffer(coefs, q, specs, fs)
    pin_c, pin_p = ctx.host_alloc(coefs.shape, np.int16), ctx.host_alloc(want.shape, np.uint8)
    try:
        pin_c[:] = coefs
        pin_p[:] = FILL
        ctx.decode_frames_submit(1, pin_c, coefs.shape[1], q, specs, 2, pin_p, fs)
        ctx.wait(1)
        assert np.array_equal(pin_p, want)
    finally:
        ctx.host_free(pin_c)
        ctx.host_free(pin_p)


# ---- the behaviour of the setting ------------------------------------------------------------------------------------
def test_switching_back_restores_the_models_bytes_and_other_contexts_are_unaffected(ctx, hvc):
    data = golden_bytes("mini.jpg")
    other = hvc.Context(0)
    try:
        assert other.arithmetic == "model"
        _, model_px = other.jpeg_decode(data)
        _, model_rgb = other.jpeg_decode_rgb(data)
        _, lib_px = ctx.jpeg_decode(data)
        _, lib_rgb = ctx.jpeg_decode_rgb(data)
        assert not np.array_equal(lib_px, model_px) and not np.array_equal(lib_rgb, model_rgb)
        assert np.abs(lib_px.astype(int) - model_px.astype(int)).max() <= 2   # two inverse DCTs of the same coefficients
        ctx.set_arithmetic("model")
        try:
            assert np.array_equal(ctx.jpeg_decode(data)[1], model_px) and np.array_equal(ctx.jpeg_decode_rgb(data)[1], model_rgb)
        finally:
            ctx.set_arithmetic("libjpeg")
        assert np.array_equal(ctx.jpeg_decode(data)[1], lib_px)
        assert np.array_equal(other.jpeg_decode(data)[1], model_px)
    finally:
        other.close()


def test_fused_scaled_and_mixed_calls_refuse_with_their_output_untouched(ctx, hvc):
    data = golden_bytes("mini.jpg")
    info = hvc.hvc.jpeg_read_header(data)
    Err = hvc.hvc.HvcError

    def refused(fn):
        with pytest.raises(Err) as e:
            fn()
        assert e.value.code == E_INVALID_ARG

    refused(lambda: ctx.jpeg_decode_yuv444(data))
    refused(lambda: ctx.jpeg_decode_scaled(data, 2))
    refused(lambda: ctx.jpeg_decode_scaled_rgb(data, 4))
    out = np.full(4 * info.pixel_bytes, FILL, dtype=np.uint8)
    refused(lambda: ctx.jpeg_decode_batch([data, data], out, 3 * 64 * 64, frames_per_chunk=1, yuv444=True))
    refused(lambda: ctx.jpeg_decode_batch([data, data], out, 3 * 64 * 64, frames_per_chunk=1, yuv444=True, gpu_entropy=True))
    refused(lambda: ctx.jpeg_decode_batch_scaled([data, data], 2, out, info.pixel_bytes))
    _, coefs = hvc.hvc.jpeg_entropy_decode(data)
    specs = [dict(blocks_w=info.layout[k].blocks_w, blocks_h=info.layout[k].blocks_h, qtab=info.layout[k].qtab,
                  coef_offset=info.layout[k].coef_offset, plane_offset=info.layout[k].plane_offset, stride=info.layout[k].stride) for k in range(3)]
    refused(lambda: ctx.decode_frames_scaled(coefs, coefs.size, info.qtab_array(), specs, 1, 2, out, info.pixel_bytes))
    refused(lambda: ctx.decode_frames_yuv444(coefs, coefs.size, info.qtab_array(), specs, 1, 64, 64, out, 3 * 64 * 64))
    refused(lambda: ctx.decode_frames_mixed(coefs, [0], [info], out, [0]))
    refused(lambda: ctx.jpeg_decode_batch_mixed([data, data], pixels=out))
    assert (out == FILL).all()


def test_a_dc_beyond_int16_is_a_range_error(ctx, hvc):
    """a 16 x 8 grey file whose second block's absolute DC is 20000 + 20000: k_islow keeps no side list"""
    q = np.ones((2, 64), dtype=np.uint16)
    dc = lambda a, b: np.array([[a] + [0] * 63, [b] + [0] * 63], dtype=np.int64)
    ok = jpeg_optimised_tables(16, 8, [(1, 1)], q, dc(20000, 20000))
    assert (ctx.jpeg_decode(ok)[1] == 255).all() and ctx.last_wide_blocks() == 2   # (S = 20000: beyond the guard)
    wide = jpeg_optimised_tables(16, 8, [(1, 1)], q, dc(20000, 40000))
    for fn in (lambda: ctx.jpeg_decode(wide), lambda: ctx.jpeg_decode_rgb(wide),
               lambda: ctx.jpeg_decode_batch([wide, wide], np.zeros(2 * 128, dtype=np.uint8), 128, frames_per_chunk=1),
               lambda: ctx.jpeg_decode_batch_rgb([wide, wide], np.zeros((2, 8, 16, 3), dtype=np.uint8), frames_per_chunk=1)):
        with pytest.raises(hvc.hvc.HvcError) as e:
            fn()
        assert e.value.code == E_RANGE
