"""Decoding at 1/2, 1/4, 1/8 size on the GPU (include/hvc_jpeg.h, "Decoding at reduced size"; csrc/hvc_scaled.hip):
k_decode_scaled and the entry points built on it against the numpy definition (tools/scaled_reference.py, which
tests/test_scaled_reference.py holds to libjpeg).  Every comparison is exact equality, and the whole output buffer is
compared: what lies between rows, planes and frames must keep its fill."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import golden_bytes
from test_gpu_rgb import frame_planes
from test_host_entropy import unusual_sampling_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rgb_reference as rgb_ref  # noqa: E402
import scaled_reference as sr  # noqa: E402
from jpeg_opt_writer import jpeg_optimised_tables  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = (2, 4, 8)
FILL = 0xA5
E_INVALID_ARG, E_ALIGNMENT, E_RANGE = -1, -4, -5


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


# ---- the block stage on records -------------------------------------------------------------------------------------
GEOMETRIES = {  # name: (planes as (blocks_w, blocks_h, table), frames)
    "420_72x40": ([(10, 6, 0), (5, 3, 1), (5, 3, 1)], 3),   # a row is no multiple of a wavefront, the planes differ in size
    "33x9": ([(33, 9, 0)], 2),                               # two tiles, the last one ragged; an odd number of blocks per row
    "one_block": ([(1, 1, 0)], 1),
    "empty_beside": ([(6, 3, 0), (0, 5, 1), (3, 2, 1)], 2),  # a component of 0 x n blocks beside real ones
}
LAYOUTS = ("tight", "odd", "aligned")


def ordinary_record(seed, planes, n_frames):
    """(tables [2][64], coefs [n_frames][coef elements]): sparse small coefficients, every block inside the int32 guard"""
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 17, size=(2, 64)).astype(np.uint16)
    fs = sum(bw * bh * 64 for bw, bh, _ in planes)
    c = rng.integers(-40, 41, size=(n_frames, max(fs // 64, 1), 64))
    c *= rng.random(size=c.shape) < 0.3
    c[..., 0] = rng.integers(-100, 101, size=c.shape[:2])
    return q, c.reshape(n_frames, -1)[:, :max(fs, 64)].astype(np.int16)


def place(planes, n, layout):
    """specs of the scaled planes and the bytes from frame to frame"""
    specs, co, po = [], 0, {"tight": 0, "odd": 1, "aligned": 4}[layout]
    for bw, bh, qt in planes:
        stride = {"tight": bw * n, "odd": bw * n + 3 + (bw * n) % 2, "aligned": up(bw * n, 4) + 8}[layout]   # odd: an odd stride
        specs.append(dict(blocks_w=bw, blocks_h=bh, qtab=qt, coef_offset=co, plane_offset=po, stride=stride))
        co += bw * bh * 64
        po += stride * bh * n + {"tight": 0, "odd": 5, "aligned": 12}[layout]
    fs = {"tight": po, "odd": po + 7 + po % 2, "aligned": up(po, 4) + 16}[layout]   # odd: an odd frame stride
    return specs, fs


def want_buffer(coefs, q, specs, fs, n):
    """the output buffer the definition gives: FILL everywhere but in the planes"""
    out = np.full((coefs.shape[0], fs), FILL, dtype=np.uint8)
    wide = 0
    for f in range(coefs.shape[0]):
        for s in specs:
            bw, bh = s["blocks_w"], s["blocks_h"]
            if not bw or not bh:
                continue
            blk = coefs[f, s["coef_offset"]:s["coef_offset"] + bw * bh * 64].reshape(bh, bw, 64)
            plane = sr.scaled_plane(blk, q[s["qtab"]], bw, bh, n)
            wide += int(np.count_nonzero(~sr.takes_int32_path(blk, q[s["qtab"]], n)))
            rows = np.arange(bh * n)[:, None] * s["stride"] + s["plane_offset"] + np.arange(bw * n)[None, :]
            out[f][rows] = plane
    return out, wide


def run(ctx, coefs, q, specs, fs, scale, device):
    """hvc_decode_frames_scaled into a buffer of FILL -> (the whole buffer, hvc_last_wide_blocks)"""
    import torch
    n_frames, coef_fs = coefs.shape
    out = np.full((n_frames, fs), FILL, dtype=np.uint8)
    if device:
        d_c, d_o = torch.from_numpy(coefs).cuda(), torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        ctx.decode_frames_scaled(d_c, coef_fs, q, specs, n_frames, scale, d_o, fs)
        ctx.synchronize()
        out = d_o.cpu().numpy()
    else:
        ctx.decode_frames_scaled(coefs, coef_fs, q, specs, n_frames, scale, out, fs)
    return out, ctx.last_wide_blocks()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_records_equal_the_definition(ctx, geometry, layout, scale, device):
    planes, n_frames = GEOMETRIES[geometry]
    q, coefs = ordinary_record(len(geometry) + scale, planes, n_frames)
    specs, fs = place(planes, 8 // scale, layout)
    want, wide = want_buffer(coefs, q, specs, fs, 8 // scale)
    got, got_wide = run(ctx, coefs, q, specs, fs, scale, device)
    assert np.array_equal(got, want)
    assert wide == 0 and got_wide == 0   # ordinary blocks: none takes the int64 branch


def guard_record(n):
    """three planes of 9 x 4 blocks with tables of 255, of 65535 and of 1: coefficients of +-32767 (dense), ordinary blocks,
    and blocks at the guard and one past it"""
    rng = np.random.default_rng(11 + n)
    q = np.stack([np.full(64, 255), np.full(64, 65535), np.ones(64)]).astype(np.uint16)
    planes = [(9, 4, 0), (9, 4, 1), (9, 4, 2)]
    c = np.zeros((3, 36, 64), dtype=np.int64)
    for k in range(2):
        c[k] = rng.choice([-32767, 32767], size=(36, 64))
        c[k, 20:] = rng.integers(-3, 4, size=(16, 64)) * (rng.random(size=(16, 64)) < 0.2)   # inside the guard with 255, outside with 65535 where not zero
    c[1, 30:] = 0
    c[1, 30:, 0] = rng.integers(-32768, 32768, size=6)   # a lone DC times 65535: beyond the guard's DC
    k = sr.spec_constants()
    if n > 1:
        p = "HVC_S%d_GUARD_" % n
        wd, wa, limit = k[p + "WD"], k[p + "WA"], k[p + "LIMIT"]
        b = 0
        for dc in (0, 1, 1000, 8192, limit // wd, min(limit // wd + 1, 32767)):
            ac = max((limit - wd * dc) // wa, 0)
            for sign, extra in ((1, 0), (-1, 0), (1, 1), (-1, 1)):
                c[2, b, 0] = sign * dc
                c[2, b, sr.ZF[8 * 7 + 7]] = -sign * (ac + extra)
                c[2, b, sr.ZF[8 * 1 + 3]] = sign * ((ac + extra) // 2)
                b += 1
        c[2, b:] = rng.integers(-1500, 1501, size=(36 - b, 64))
    else:
        c[2] = rng.integers(-32768, 32768, size=(36, 64))
    return q, planes, c.reshape(1, -1).astype(np.int16)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["tight", "aligned"])
@pytest.mark.parametrize("scale", SCALES)
def test_both_sides_of_the_guard_and_the_extremes(ctx, scale, layout, device):
    n = 8 // scale
    q, planes, coefs = guard_record(n)
    coefs = np.concatenate([coefs, coefs[:, ::-1].reshape(-1, 64)[:, ::-1].reshape(1, -1)])   # a second frame: the blocks in reverse order
    specs, fs = place(planes, n, layout)
    want, wide = want_buffer(coefs, q, specs, fs, n)
    got, got_wide = run(ctx, coefs, q, specs, fs, scale, device)
    assert np.array_equal(got, want)
    assert got_wide == wide
    assert (wide > 40) == (n > 1)   # both branches are taken (N = 1 has one)
    blocks = coefs.size // 64
    assert n == 1 or wide < blocks - 40


def test_scale_1_is_decode_frames(ctx, hvc):
    planes, n_frames = GEOMETRIES["420_72x40"]
    q, coefs = ordinary_record(5, planes, n_frames)
    specs, fs = place(planes, 8, "tight")
    a, b = np.zeros((n_frames, fs), dtype=np.uint8), np.ones((n_frames, fs), dtype=np.uint8)
    ctx.decode_frames(coefs, coefs.shape[1], q, specs, n_frames, a, fs)
    ctx.decode_frames_scaled(coefs, coefs.shape[1], q, specs, n_frames, 1, b, fs)
    assert np.array_equal(a, b)
    odd = [dict(s, stride=s["stride"] + 1) for s in specs]   # ... with hvc_decode_frames' alignment rules
    with pytest.raises(hvc.hvc.HvcError) as e:
        ctx.decode_frames_scaled(coefs, coefs.shape[1], q, odd, 1, 1, b, fs + 100)
    assert e.value.code == E_ALIGNMENT


def test_profiling_ring_takes_a_device_call(ctx):
    import torch
    planes, n_frames = GEOMETRIES["33x9"]
    q, coefs = ordinary_record(6, planes, n_frames)
    specs, fs = place(planes, 4, "tight")
    d_c, d_o = torch.from_numpy(coefs).cuda(), torch.zeros((n_frames, fs), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.set_profiling(True)
    try:
        ctx.decode_frames_scaled(d_c, coefs.shape[1], q, specs, n_frames, 2, d_o, fs)
        assert ctx.last_kernel_ms() > 0
    finally:
        ctx.set_profiling(False)


# ---- files ----------------------------------------------------------------------------------------------------------
def definition_of_file(hvc, jpg, scale, restart_markers=False):
    """(scaled info, the scaled padded planes of the file by the numpy definition over the host reader's record)"""
    info, coefs = hvc.hvc.jpeg_entropy_decode(jpg, restart_markers=restart_markers)
    n = 8 // scale
    planes = []
    for k in range(info.n_comp):
        L = info.layout[k]
        blk = coefs[L.coef_offset:L.coef_offset + L.blocks_w * L.blocks_h * 64]
        planes.append(sr.scaled_plane(blk, info.qtab_array()[L.qtab], L.blocks_w, L.blocks_h, n))
    return hvc.hvc.jpeg_scaled_info(info, scale), planes


def sampling_of(info):
    if info.n_comp == 1:
        return 400
    key = (info.comp[0].decoded_width // info.comp[1].decoded_width, info.comp[0].decoded_height // info.comp[1].decoded_height)
    return {(2, 2): 420, (2, 1): 422, (1, 1): 444}[key]


@pytest.fixture(scope="module")
def batch_files(hvc):
    """8 files of 64 x 48 4:2:0 with one set of quantiser tables: six plain, one with its own optimised Huffman tables --
    and the same eight frames written with restart intervals"""
    c = hvc.Context(0)
    try:
        frames = [frame_planes(300 + 3 * f, 64, 48, 420) for f in range(8)]
        plain = [c.jpeg_encode(*fr, 64, 48, 420, 80) for fr in frames]
        info, coefs = hvc.hvc.jpeg_entropy_decode(plain[5])
        plain[5] = jpeg_optimised_tables(64, 48, 420, info.qtab_array(), coefs)
        c.set_restart_interval(5)
        rst = [c.jpeg_encode(*fr, 64, 48, 420, 80) for fr in frames]
    finally:
        c.close()
    return plain, rst


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("restart", [False, True], ids=["plain", "restart"])
def test_batch_pipelines_and_single_files(hvc, batch_files, scale, restart):
    """the compact DC array: the GPU reader's pipeline (chunks of 3: the ring goes round) against the host reader's, against
    the single-file call and against the definition; to host and to device memory"""
    import torch
    jpegs = batch_files[1 if restart else 0]
    c = hvc.Context(0)
    try:
        c.set_restart_markers(restart)
        want = []
        for j in jpegs:
            sinfo, planes = definition_of_file(hvc, j, scale, restart)
            info, px = c.jpeg_decode_scaled(j, scale)
            assert (info.width, info.height, info.pixel_bytes) == (sinfo.width, sinfo.height, sinfo.pixel_bytes)
            assert all(bytes(info.layout[k]) == bytes(sinfo.layout[k]) and bytes(info.comp[k]) == bytes(sinfo.comp[k]) for k in range(3))
            assert np.array_equal(px, np.concatenate([p.reshape(-1) for p in planes]))
            assert c.last_wide_blocks() == 0
            want.append(px)
        want = np.stack(want)
        fs = want.shape[1] + 3   # any frame stride
        for gpu_entropy in (True, False):
            host = np.full((len(jpegs), fs), FILL, dtype=np.uint8)
            st = c.jpeg_decode_batch_scaled(jpegs, scale, host, fs, threads=2, frames_per_chunk=3, gpu_entropy=gpu_entropy)
            assert st.chunks == 3
            # the GPU reader took every chunk (no host entropy decoding: nothing fell back to the host reader's pipeline), so
            # the kernels that read the compact DC array ran; the host reader's pipeline reports its entropy time
            assert (st.entropy_ms_sum == 0) if gpu_entropy else (st.entropy_ms_sum > 0)
            assert np.array_equal(host[:, :-3], want) and (host[:, -3:] == FILL).all()
            dev = torch.full((len(jpegs), fs), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            st = c.jpeg_decode_batch_scaled(jpegs, scale, dev, fs, threads=2, frames_per_chunk=3, gpu_entropy=gpu_entropy)
            c.synchronize()
            assert (st.entropy_ms_sum == 0) if gpu_entropy else (st.entropy_ms_sum > 0)
            assert np.array_equal(dev.cpu().numpy(), host)
    finally:
        c.close()


def test_a_scaled_batch_takes_one_ring_entry_per_chunk(hvc, batch_files):
    """with profiling on, every chunk's scaled block stage is timed: what tools/bench_scaled.py reads k_decode_scaled's time
    with and without the compact DC array from"""
    c = hvc.Context(0)
    try:
        out = np.zeros((8, 72), dtype=np.uint8)
        for gpu_entropy in (True, False):
            c.set_profiling(True)
            st = c.jpeg_decode_batch_scaled(batch_files[0], 8, out, 72, threads=2, frames_per_chunk=3, gpu_entropy=gpu_entropy)
            ms = c.kernel_ms_history(st.chunks)
            assert len(ms) == 3 and all(t > 0 for t in ms)
            with pytest.raises(hvc.hvc.HvcError):
                c.kernel_ms_history(st.chunks + 1)
    finally:
        c.close()


def rgb_files(ctx):
    y, u, v = frame_planes(41, 70, 38, 420)
    yield "420 70x38", ctx.jpeg_encode(y, u, v, 70, 38, 420, 85), (2, 4)   # odd scaled sizes: 35 x 19, 18 x 10
    yield "422", ctx.jpeg_encode(*frame_planes(42, 52, 44, 422), 52, 44, 422, 85), SCALES
    yield "444", ctx.jpeg_encode(*frame_planes(43, 45, 53, 444), 45, 53, 444, 85), SCALES
    yield "grey", unusual_sampling_file([(1, 1)], 97, 51, 3)[0], SCALES


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_scaled_rgb_is_the_colour_definition_over_the_scaled_planes(ctx, hvc, layout):
    for name, jpg, scales in rgb_files(ctx):
        for scale in scales:
            sinfo, planes = definition_of_file(hvc, jpg, scale)
            p = planes + [None, None]
            want = rgb_ref.planes_to_rgb(p[0], p[1], p[2], sampling_of(sinfo), sinfo.width, sinfo.height, layout)
            info, got = ctx.jpeg_decode_scaled_rgb(jpg, scale, layout)
            assert (info.width, info.height) == (sinfo.width, sinfo.height), name
            assert got.shape == hvc.hvc.rgb_shape(layout, sinfo.width, sinfo.height) and np.array_equal(got, want), (name, scale)


def test_errors(ctx, hvc):
    L = hvc.lib()
    jpg = golden_bytes("mini.jpg")
    info = hvc.hvc.JpegInfo()
    out = np.full(64 * 64 * 3, FILL, dtype=np.uint8)
    planes, n_frames = GEOMETRIES["420_72x40"]
    q, coefs = ordinary_record(5, planes, n_frames)
    specs, fs = place(planes, 4, "tight")
    comps = hvc.hvc.components(specs)
    frames = lambda s: L.hvc_decode_frames_scaled(ctx._h, coefs.ctypes.data, coefs.shape[1], q.ctypes.data, 2, comps, 3, n_frames, s,
                                                 out.ctypes.data, fs, 0)
    ptrs, sizes = (C.c_void_p * 1)(C.cast(C.c_char_p(jpg), C.c_void_p)), (C.c_size_t * 1)(len(jpg))
    calls = {
        "frames": frames,
        "file": lambda s: L.hvc_jpeg_decode_scaled(ctx._h, jpg, len(jpg), s, C.byref(info), out.ctypes.data, out.size),
        "rgb": lambda s: L.hvc_jpeg_decode_scaled_rgb(ctx._h, jpg, len(jpg), s, C.byref(info), out.ctypes.data, out.size, 0, 0),
        "batch": lambda s: L.hvc_jpeg_decode_batch_scaled(ctx._h, ptrs, sizes, 1, 1, 0, 0, s, out.ctypes.data, out.size, 0, None),
        "batch_gpu": lambda s: L.hvc_jpeg_decode_batch_scaled(ctx._h, ptrs, sizes, 1, 1, 0, 1, s, out.ctypes.data, out.size, 0, None),
    }
    for name, call in calls.items():   # a scale_denom that is none of 1, 2, 4, 8
        for s in (0, 3, 16, -2):
            assert call(s) == E_INVALID_ARG, (name, s)
    assert (out == FILL).all()
    ctx.set_arithmetic("hardcaml")   # no RTL form of the scaled path: refused, output untouched
    try:
        for name, call in calls.items():
            for s in SCALES:
                assert call(s) == E_INVALID_ARG, (name, s)
        assert (out == FILL).all() and info.width == 0
    finally:
        ctx.set_arithmetic("model")
    # a pixel_cap / rgb_cap that is too small
    need = hvc.hvc.jpeg_scaled_info(hvc.hvc.jpeg_read_header(jpg), 2).pixel_bytes
    assert L.hvc_jpeg_decode_scaled(ctx._h, jpg, len(jpg), 2, C.byref(info), out.ctypes.data, need - 1) == E_INVALID_ARG
    assert L.hvc_jpeg_decode_scaled_rgb(ctx._h, jpg, len(jpg), 2, C.byref(info), out.ctypes.data, 32 * 32 * 3 - 1, 0, 0) == E_INVALID_ARG
    assert L.hvc_jpeg_decode_batch_scaled(ctx._h, ptrs, sizes, 1, 1, 0, 0, 2, out.ctypes.data, need - 1, 0, None) == E_INVALID_ARG
    assert (out == FILL).all()
    assert L.hvc_jpeg_decode_scaled(ctx._h, jpg, len(jpg), 2, C.byref(info), out.ctypes.data, need) == 0


def test_a_dc_beyond_int16_is_a_range_error(ctx, hvc):
    """a 16 x 8 grey file whose second block's absolute DC is 20000 + 20000: the scaled block stage keeps no side list"""
    q = np.ones((2, 64), dtype=np.uint16)
    dc = lambda a, b: np.array([[a] + [0] * 63, [b] + [0] * 63], dtype=np.int64)
    ok = jpeg_optimised_tables(16, 8, [(1, 1)], q, dc(20000, 20000))
    assert ctx.jpeg_decode_scaled(ok, 8)[1].tolist() == [255, 255]
    wide = jpeg_optimised_tables(16, 8, [(1, 1)], q, dc(20000, 40000))
    with pytest.raises(hvc.hvc.HvcError) as e:   # (the file is what it is meant to be: the record-returning reader refuses it)
        hvc.hvc.jpeg_entropy_decode(wide)
    assert e.value.code == E_RANGE
    for s in SCALES:
        with pytest.raises(hvc.hvc.HvcError) as e:
            ctx.jpeg_decode_scaled(wide, s)
        assert e.value.code == E_RANGE
        with pytest.raises(hvc.hvc.HvcError) as e:
            ctx.jpeg_decode_scaled_rgb(wide, s)
        assert e.value.code == E_RANGE
        out = np.zeros(64, dtype=np.uint8)
        for gpu_entropy in (False, True):
            with pytest.raises(hvc.hvc.HvcError) as e:
                ctx.jpeg_decode_batch_scaled([wide, wide], s, out, 32, gpu_entropy=gpu_entropy)
            assert e.value.code == E_RANGE


def test_cli_round_trip(tmp_path, ctx, hvc):
    from video_coding_amd.__main__ import main
    jpg = golden_bytes("Mouse480.jpg")
    (tmp_path / "in.jpg").write_bytes(jpg)
    main(["model", "decode", "frame", str(tmp_path / "in.jpg"), str(tmp_path / "out.yuv"), "-scale", "4"])
    info, pixels = ctx.jpeg_decode_scaled(jpg, 4)
    assert (tmp_path / "out.yuv").read_bytes() == hvc.hvc.jpeg_get_cropped_planes(info, pixels).tobytes()
    main(["model", "decode", "frame", str(tmp_path / "in.jpg"), str(tmp_path / "out.ppm"), "-scale", "4", "-rgb"])
    info, image = ctx.jpeg_decode_scaled_rgb(jpg, 4)
    assert (tmp_path / "out.ppm").read_bytes() == b"P6\n%d %d\n255\n" % (info.width, info.height) + image.tobytes()
    with pytest.raises(SystemExit):
        main(["model", "decode", "frame", str(tmp_path / "in.jpg"), str(tmp_path / "x"), "-scale", "2", "-yuv444"])


def test_the_measured_kernels_are_the_parents(hvc):
    """csrc/hvc_scaled.hip is a translation unit of its own: the kernel id the counters are keyed on stays"""
    assert hvc.hvc.kernel_source_id() == hvc.hvc.kernel_build_id() == "b746d7b6f0f2"
