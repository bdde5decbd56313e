"""Restart intervals (DRI + RSTn) written ON THE GPU: hvc_huffman_encode_frames_restart (the k_*_rst passes of
csrc/hvc_huff.hip) and hvc_set_restart_interval on hvc_jpeg_encode, hvc_jpeg_encode_batch and hvc_jpeg_encode_batch_gpu.
The yardstick is the host composition, hvc_jpeg_entropy_encode_restart over the frame's coefficient record
(tests/test_restart_encode.py holds that to the pure-Python writer); the files then go back through the GPU reader with
hvc_set_restart_markers on, which closes the loop between this library's writer and its reader."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from conftest import GOLDEN as _GOLDEN, golden_json
from helpers import checksum_records, synth_pixels
from oracle import orc

pytestmark = pytest.mark.gpu

RST = re.compile(rb"\xff[\xd0-\xd7]")


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(hvc):
    c = hvc.Context(0)
    yield c
    c.close()


def planes_of(seed, w, h, chroma):
    cw, ch = orc.chroma_dims(chroma, w, h)
    r8 = lambda x: (x + 7) // 8 * 8
    y = synth_pixels(seed, r8(h), r8(w))[:h, :w]
    u = synth_pixels(seed + 1, r8(ch), r8(cw))[:ch, :cw]
    v = synth_pixels(seed + 2, r8(ch), r8(cw))[:ch, :cw]
    return np.ascontiguousarray(y), np.ascontiguousarray(u), np.ascontiguousarray(v)


def record_of(seed, w, h, chroma, quality):
    y, u, v = planes_of(seed, w, h, chroma)
    _, coefs = orc.encode_yuv(y, u, v, w, h, chroma, quality, want_coefs=True)
    return np.concatenate([c.reshape(-1) for c in coefs]).astype(np.int16)


def mcus(info):
    c0 = info.comp[0]
    return (c0.decoded_width // (8 * c0.hscale)) * (c0.decoded_height // (8 * c0.vscale))


def frames_of(n, w, h, chroma, base):
    out = []
    for f in range(n):
        y, u, v = planes_of(base + 13 * f, w, h, chroma)
        out.append((y, u, v, np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])))
    return out


# -- 7: the coder on resident records --------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w,h,chroma", [(72, 40, 420), (130, 66, 422), (33, 17, 444), (200, 72, 444)])
def test_encode_frames_restart_per_frame(ctx, hvc, w, h, chroma, device):
    """24 frames of different content and quality in one call, default and optimised tables, a range of intervals: each
    frame's segment (markers included) equals the host function's, the specs hvc_huffman_optimal_tables_restart's"""
    n = 24
    info = hvc.hvc.jpeg_encoder_layout(w, h, chroma, 75)
    stride = (info.coef_count + 7) // 8 * 8 + 8       # records not back to back
    recs = np.zeros((n, stride), dtype=np.int16)
    for f in range(n):
        recs[f, :info.coef_count] = record_of(2000 + 17 * f, w, h, chroma, 5 + (f * 37) % 95)
    if device:
        import torch
        coefs = torch.from_numpy(recs.reshape(-1)).cuda()
    else:
        coefs = recs.reshape(-1)
    n_mcu = mcus(info)
    plain = ctx.huffman_encode_frames(info, coefs, stride, n)
    mw = n_mcu // (info.comp[0].decoded_height // (8 * info.comp[0].vscale))
    for ri in sorted({1, 2, 3, 7, mw, n_mcu - 1, n_mcu, n_mcu + 5, 65535}):
        segs = ctx.huffman_encode_frames(info, coefs, stride, n, restart_interval=ri)
        osegs, specs = ctx.huffman_encode_frames_optimised(info, coefs, stride, n, restart_interval=ri)
        head = hvc.hvc.jpeg_header(info, restart_interval=ri)
        for f in range(n):
            rec = recs[f, :info.coef_count]
            want = hvc.hvc.jpeg_entropy_encode(info, rec, restart_interval=ri)
            assert segs[f] == want[len(head):-2], "Ri %d, frame %d" % (ri, f)
            want_specs = hvc.hvc.huffman_optimal_tables(info, rec, restart_interval=ri)
            assert specs[f] == want_specs, "Ri %d, frame %d" % (ri, f)
            ohead = hvc.hvc.jpeg_header(info, want_specs, restart_interval=ri)
            assert osegs[f] == hvc.hvc.jpeg_entropy_encode(info, rec, want_specs, restart_interval=ri)[len(ohead):-2], (ri, f)
            if ri >= n_mcu:
                assert segs[f] == plain[f]
            else:
                assert len(RST.findall(segs[f])) == -(-n_mcu // ri) - 1
    assert ctx.huffman_encode_frames(info, coefs, stride, n) == plain  # and the plain coder is what it was


def test_stuffed_ff_in_front_of_a_marker_on_the_gpu(ctx, hvc):
    """the random records of tests/test_restart_encode.py whose expected bytes hold FF 00 FF Dn (a pad byte of 0xFF)"""
    from test_restart_encode import random_record
    for chroma, sampling in ((420, [(2, 2), (1, 1), (1, 1)]), (444, [(1, 1)] * 3)):
        info = hvc.hvc.jpeg_encoder_layout(200, 72, chroma, 50)
        recs = np.stack([random_record(sampling, 200, 72, seed)[0] for seed in range(4)])
        assert recs.shape[1] == info.coef_count and info.coef_count % 8 == 0
        segs = ctx.huffman_encode_frames(info, recs.reshape(-1), info.coef_count, 4, restart_interval=1)
        head = hvc.hvc.jpeg_header(info, restart_interval=1)
        places = 0
        for f in range(4):
            want = hvc.hvc.jpeg_entropy_encode(info, recs[f], restart_interval=1)[len(head):-2]
            assert segs[f] == want, f
            places += len(re.findall(rb"\xff\x00\xff[\xd0-\xd7]", want))
        assert places >= 1


def test_range_and_argument_errors(ctx, hvc):
    L = hvc.lib()
    info = hvc.hvc.jpeg_encoder_layout(16, 8, 444, 50)
    rec = np.zeros(info.coef_count, dtype=np.int16).reshape(3, 2, 64)
    rec[:, 0, 0], rec[:, 1, 0] = 2047, -2047  # category 12 in the plain scan, 11 from zero
    flat = np.ascontiguousarray(rec.reshape(-1))
    out = np.empty(65536, dtype=np.uint8)
    offs = np.zeros(2, dtype=np.uint64)
    specs = (hvc.hvc.HuffSpec * 4)()

    def call(ri, tables, sp=specs, n=1):
        return L.hvc_huffman_encode_frames_restart(ctx._h, C.byref(info), flat.ctypes.data, info.coef_count, n, ri, tables,
                                                   out.ctypes.data, out.size, offs.ctypes.data, sp, 0)
    assert call(0, 0) == -5 and call(2, 0) == -5 and call(0, 1) == -5
    assert call(1, 0) == 0 and call(1, 1) == 0
    want = hvc.hvc.jpeg_entropy_encode(info, flat, restart_interval=1)
    head = hvc.hvc.jpeg_header(info, restart_interval=1)
    assert call(1, 0, None) == 0 and out[:int(offs[1])].tobytes() == want[len(head):-2]
    rec[:, 0, 0], rec[:, 1, 0] = 1000, 2500  # category 11 in the plain scan, 12 from zero
    flat[:] = rec.reshape(-1)
    assert call(0, 0) == 0 and call(1, 0) == -5 and call(1, 1) == -5
    for ri in (-1, 65536):
        assert call(ri, 0) == -1
    assert call(1, 2) == -1 and call(1, -1) == -1
    assert call(1, 1, None) == -1  # optimised tables need somewhere to put the specs


def test_set_get_round_trip(ctx, hvc):
    L = hvc.lib()
    assert ctx.restart_interval == 0
    ctx.set_restart_interval(65535)
    assert ctx.restart_interval == 65535
    for bad in (-1, 65536, 1 << 30):
        assert L.hvc_set_restart_interval(ctx._h, bad) == -1
    assert ctx.restart_interval == 65535
    ctx.set_restart_interval(0)
    v = C.c_int(-5)
    assert L.hvc_get_restart_interval(ctx._h, C.byref(v)) == 0 and v.value == 0
    assert L.hvc_get_restart_interval(ctx._h, None) == -1


# -- 8, 9: the file entry points, and the files back through the GPU reader ---------------------------------------------------

def check_file_entry_points(hvc, w, h, chroma, quality, n, chunk, base, ri, arith="model"):
    frames = frames_of(n, w, h, chroma, base)
    raw = [f[3] for f in frames]
    info = hvc.hvc.jpeg_encoder_layout(w, h, chroma, quality)
    ctx = hvc.Context(0)  # a context whose setting has never been touched
    try:
        ctx.set_encode_arithmetic(arith)
        before = [ctx.jpeg_encode(y, u, v, w, h, chroma, quality) for y, u, v, _ in frames]
        before_batch, _ = ctx.jpeg_encode_batch(raw, w, h, chroma, quality, threads=4, frames_per_chunk=chunk)
        before_gpu, _ = ctx.jpeg_encode_batch(raw, w, h, chroma, quality, threads=4, frames_per_chunk=chunk, gpu_entropy=True)
        assert before == before_batch == before_gpu
        recs = []
        for jpg in before:
            _, rec = hvc.hvc.jpeg_entropy_decode(jpg)
            recs.append(np.ascontiguousarray(rec.reshape(-1)[:info.coef_count]))
            assert hvc.hvc.jpeg_entropy_encode(info, recs[-1]) == jpg
        files = {}
        for tables in ("default", "optimised"):
            ctx.set_huffman_tables(tables)
            ctx.set_restart_interval(ri)
            assert ctx.restart_interval == ri
            want = [hvc.hvc.jpeg_entropy_encode(info, r, None if tables == "default" else "optimised", restart_interval=ri)
                    for r in recs]
            single = [ctx.jpeg_encode(y, u, v, w, h, chroma, quality) for y, u, v, _ in frames]
            batch, _ = ctx.jpeg_encode_batch(raw, w, h, chroma, quality, threads=4, frames_per_chunk=chunk)
            batch_gpu, _ = ctx.jpeg_encode_batch(raw, w, h, chroma, quality, threads=4, frames_per_chunk=chunk, gpu_entropy=True)
            for f in range(n):
                assert single[f] == want[f], "hvc_jpeg_encode, %s, frame %d" % (tables, f)
                assert batch[f] == want[f], "hvc_jpeg_encode_batch, %s, frame %d" % (tables, f)
                assert batch_gpu[f] == want[f], "hvc_jpeg_encode_batch_gpu, %s, frame %d" % (tables, f)
            files[tables] = want
            ctx.set_restart_interval(0)
            if tables == "default":  # back to 0: the bytes of before the setting was ever touched
                assert [ctx.jpeg_encode(y, u, v, w, h, chroma, quality) for y, u, v, _ in frames] == before
                assert ctx.jpeg_encode_batch(raw, w, h, chroma, quality, threads=4, frames_per_chunk=chunk)[0] == before
                assert ctx.jpeg_encode_batch(raw, w, h, chroma, quality, threads=4, frames_per_chunk=chunk,
                                             gpu_entropy=True)[0] == before
        ctx.set_huffman_tables("default")
        # the loop closed on the device: the GPU reader with the extension on
        ctx.set_restart_markers(True)
        pix_bytes = hvc.hvc.jpeg_read_header(before[0]).pixel_bytes
        plain_pixels = np.zeros(n * pix_bytes, dtype=np.uint8)
        ctx.jpeg_decode_batch(before, plain_pixels, pix_bytes, threads=4, frames_per_chunk=4, gpu_entropy=True)
        for tables, fs in files.items():
            for device in (False, True):
                _, got, used = ctx.jpeg_entropy_decode_gpu(fs, device=device)
                assert used == 1, tables
                for f in range(n):
                    assert np.array_equal(got[f][:info.coef_count], recs[f]), (tables, f)
            pixels = np.zeros(n * pix_bytes, dtype=np.uint8)
            st = ctx.jpeg_decode_batch(fs, pixels, pix_bytes, threads=4, frames_per_chunk=4, gpu_entropy=True)
            assert st.entropy_ms_sum == 0, tables
            assert np.array_equal(pixels, plain_pixels), tables
    finally:
        ctx.close()
    return before, files


@pytest.mark.parametrize("w,h,chroma,quality,ri", [(64, 64, 420, 75, 1), (130, 66, 422, 40, 5), (72, 40, 444, 90, 2),
                                                   (480, 320, 420, 60, 30), (200, 72, 444, 50, 7)])
def test_file_entry_points_agree_and_read_back_on_the_gpu(hvc, w, h, chroma, quality, ri):
    before, files = check_file_entry_points(hvc, w, h, chroma, quality, 10, chunk=3, base=w + h, ri=ri)
    assert all(len(a) > len(b) for a, b in zip(files["default"], before))  # DRI, pad bits, markers


def test_with_hardcaml_encode_arithmetic(hvc):
    before, _ = check_file_entry_points(hvc, 96, 64, 420, 80, 9, chunk=4, base=5, ri=3, arith="hardcaml")
    y, u, v = planes_of(5, 96, 64, 420)
    assert before[0] != orc.encode_yuv(y, u, v, 96, 64, 420, 80)  # the records are the RTL twin's, not the model's


# -- 10: full size ----------------------------------------------------------------------------------------------------------

def test_config5_size_batch_gpu_with_one_mcu_row_per_interval(ctx, hvc):
    """16 4K 4:2:0 frames at q75 (config 5's shape and frame generator) through hvc_jpeg_encode_batch_gpu with Ri = 240 =
    one MCU row: every file equals the host composition of its own record (which the plain file carries), the files' K5
    checksums on the device are numpy's over the host composition, and the GPU reader returns the records"""
    from video_coding_amd.synth import synth_pixels as synth
    W, H, n, ri = 3840, 2160, 16, 240
    frames = []
    for f in range(n):
        y, u, v = synth(110 + f, H, W), synth(120 + f, H // 2, W // 2), synth(130 + f, H // 2, W // 2)
        frames.append(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]))
    info = hvc.hvc.jpeg_encoder_layout(W, H, 420, 75)
    assert mcus(info) == 240 * 135
    plain, _ = ctx.jpeg_encode_batch(frames, W, H, 420, 75, threads=8, frames_per_chunk=4, gpu_entropy=True)
    ctx.set_restart_interval(ri)
    try:
        got, _ = ctx.jpeg_encode_batch(frames, W, H, 420, 75, threads=8, frames_per_chunk=4, gpu_entropy=True)
    finally:
        ctx.set_restart_interval(0)
    recs, want = [], []
    for f in range(n):
        _, rec = hvc.hvc.jpeg_entropy_decode(plain[f])
        recs.append(np.ascontiguousarray(rec.reshape(-1)[:info.coef_count]))
        want.append(hvc.hvc.jpeg_entropy_encode(info, recs[-1], restart_interval=ri))
        assert got[f] == want[-1], "frame %d" % f
        assert len(RST.findall(got[f][len(hvc.hvc.jpeg_header(info, restart_interval=ri)):])) == 134
    size = (max(map(len, want)) + 7) // 8 * 8
    pad = lambda files: np.stack([np.frombuffer(j + bytes(size - len(j)), dtype=np.uint8) for j in files])
    assert np.array_equal(ctx.checksum_records(pad(got), size, n), checksum_records(pad(want)))
    ctx.set_restart_markers(True)
    try:
        _, back, used = ctx.jpeg_entropy_decode_gpu(got)
    finally:
        ctx.set_restart_markers(False)
    assert used == 1
    for f in range(n):
        assert np.array_equal(back[f][:info.coef_count], recs[f]), f


# -- 11: the command line ---------------------------------------------------------------------------------------------------

def test_cli_restart_interval_round_trip(tmp_path):
    from video_coding_amd.__main__ import main
    cli = lambda *argv: main([str(a) for a in argv])
    c = golden_json("g4_psnr_pins.json")["cases"][0]
    src, size = pathlib.Path(_GOLDEN) / c["file"], "%dx%d" % (c["width"], c["height"])
    plain, rst = tmp_path / "plain.jpg", tmp_path / "rst.jpg"
    out_plain, out_rst, out_first = tmp_path / "plain.yuv", tmp_path / "rst.yuv", tmp_path / "first.yuv"
    cli("model", "encode", "frame", src, size, plain, "-quality", c["quality"], "-chroma", c["chroma"])
    cli("model", "encode", "frame", src, size, rst, "-quality", c["quality"], "-chroma", c["chroma"], "-restart-interval", 5)
    cli("model", "decode", "frame", plain, out_plain)
    cli("model", "decode", "frame", rst, out_rst, "-restart-markers")
    assert out_rst.read_bytes() == out_plain.read_bytes()
    data = rst.read_bytes()
    assert b"\xff\xdd\x00\x04\x00\x05\xff\xda" in data and len(data) > len(plain.read_bytes())
    # without the flag the reader is the model's: the first interval only
    cli("model", "decode", "frame", rst, out_first)
    assert out_first.read_bytes() != out_plain.read_bytes()
