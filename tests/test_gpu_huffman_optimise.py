"""Per-file optimised Huffman tables on the GPU: hvc_huffman_encode_frames_optimised (k_huff_hist + k_huff_build + the
coder's passes with per-frame tables) and hvc_set_huffman_tables(HVC_HUFF_OPTIMISED) on hvc_jpeg_encode,
hvc_jpeg_encode_batch and hvc_jpeg_encode_batch_gpu.  The yardstick is the host composition: the frame's coefficient
record through hvc_huffman_optimal_tables and hvc_jpeg_entropy_encode_tables (tests/test_huffman_optimise.py holds those
to the Annex K.2 writer)."""
import numpy as np
import pytest

from helpers import synth_pixels
from oracle import orc

pytestmark = pytest.mark.gpu


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


def host_file(hvc, info, rec):
    """the host composition: the record's own tables, then the whole file"""
    specs = hvc.hvc.huffman_optimal_tables(info, rec)
    return specs, hvc.hvc.jpeg_entropy_encode(info, rec, specs)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w,h,chroma", [(72, 40, 420), (130, 66, 422), (33, 17, 444)])
def test_encode_frames_optimised_per_frame(ctx, hvc, w, h, chroma, device):
    """64 frames whose content (and quality) differ: every frame's specs and segment equal the host's for that frame --
    a table shared across frames or a frame-stride error shows up as a mismatch"""
    n = 64
    info = hvc.hvc.jpeg_encoder_layout(w, h, chroma, 75)
    stride = (info.coef_count + 7) // 8 * 8 + 8       # records not back to back
    recs = np.zeros((n, stride), dtype=np.int16)
    for f in range(n):
        recs[f, :info.coef_count] = record_of(1000 + 17 * f, w, h, chroma, 5 + (f * 37) % 95)
    if device:
        import torch
        coefs = torch.from_numpy(recs.reshape(-1)).cuda()
    else:
        coefs = recs.reshape(-1)
    segs, specs = ctx.huffman_encode_frames_optimised(info, coefs, stride, n)
    distinct = set()
    for f in range(n):
        rec = recs[f, :info.coef_count]
        want_specs, jpg = host_file(hvc, info, rec)
        assert specs[f] == want_specs, "frame %d" % f
        head = hvc.hvc.jpeg_header(info, want_specs)
        assert segs[f] == jpg[len(head):-2], "frame %d" % f
        distinct.add(repr(want_specs))
    assert len(distinct) > n // 2  # the frames really have tables of their own


def frames_of(n, w, h, chroma, base):
    out = []
    for f in range(n):
        y, u, v = planes_of(base + 13 * f, w, h, chroma)
        out.append((y, u, v, np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])))
    return out


def check_file_entry_points(ctx, hvc, w, h, chroma, quality, n, chunk, base):
    frames = frames_of(n, w, h, chroma, base)
    info = hvc.hvc.jpeg_encoder_layout(w, h, chroma, quality)
    # the coefficient records of the context's block stage (model or Hardcaml arithmetic), through the default coder
    ctx.set_huffman_tables("default")
    default = [ctx.jpeg_encode(y, u, v, w, h, chroma, quality) for y, u, v, _ in frames]
    recs = []
    for jpg in default:
        _, rec = hvc.hvc.jpeg_entropy_decode(jpg)
        recs.append(np.ascontiguousarray(rec.reshape(-1)[:info.coef_count]))
        assert hvc.hvc.jpeg_entropy_encode(info, recs[-1]) == jpg
    ctx.set_huffman_tables("optimised")
    assert ctx.huffman_tables == "optimised"
    want = [host_file(hvc, info, r)[1] for r in recs]
    single = [ctx.jpeg_encode(y, u, v, w, h, chroma, quality) for y, u, v, _ in frames]
    batch, _ = ctx.jpeg_encode_batch([f[3] for f in frames], w, h, chroma, quality, threads=4, frames_per_chunk=chunk)
    batch_gpu, _ = ctx.jpeg_encode_batch([f[3] for f in frames], w, h, chroma, quality, threads=4, frames_per_chunk=chunk,
                                         gpu_entropy=True)
    for f in range(n):
        assert single[f] == want[f], "hvc_jpeg_encode, frame %d" % f
        assert batch[f] == want[f], "hvc_jpeg_encode_batch, frame %d" % f
        assert batch_gpu[f] == want[f], "hvc_jpeg_encode_batch_gpu, frame %d" % f
    ctx.set_huffman_tables("default")
    return info, default, want


@pytest.mark.parametrize("w,h,chroma,quality", [(64, 64, 420, 75), (130, 66, 422, 40), (33, 17, 444, 90)])
def test_file_entry_points_agree_and_decode_to_the_same_pixels(ctx, hvc, w, h, chroma, quality):
    n = 20
    info, default, opt = check_file_entry_points(ctx, hvc, w, h, chroma, quality, n, chunk=3, base=w + h)
    if w >= 64 and h >= 64:
        assert sum(map(len, opt)) < sum(map(len, default))
    pix_bytes = hvc.hvc.jpeg_read_header(default[0]).pixel_bytes
    for gpu_entropy in (False, True):
        got = {}
        for name, files in (("default", default), ("optimised", opt)):
            pixels = np.zeros(n * pix_bytes, dtype=np.uint8)
            ctx.jpeg_decode_batch(files, pixels, pix_bytes, threads=4, frames_per_chunk=4, gpu_entropy=gpu_entropy)
            got[name] = pixels
        assert np.array_equal(got["default"], got["optimised"])
    for a, b in zip(orc.decode_a_frame(opt[0]), orc.decode_a_frame(default[0])):
        assert np.array_equal(a, b)


def test_default_after_optimised_is_byte_identical(ctx, hvc):
    w, h, chroma, q = 80, 48, 420, 60
    frames = frames_of(6, w, h, chroma, 77)
    info = hvc.hvc.jpeg_encoder_layout(w, h, chroma, q)
    ctx.set_huffman_tables("optimised")
    opt = [ctx.jpeg_encode(y, u, v, w, h, chroma, q) for y, u, v, _ in frames]
    ctx.set_huffman_tables("default")
    assert ctx.huffman_tables == "default"
    single = [ctx.jpeg_encode(y, u, v, w, h, chroma, q) for y, u, v, _ in frames]
    batch, _ = ctx.jpeg_encode_batch([f[3] for f in frames], w, h, chroma, q, threads=2, frames_per_chunk=2)
    batch_gpu, _ = ctx.jpeg_encode_batch([f[3] for f in frames], w, h, chroma, q, threads=2, frames_per_chunk=2,
                                         gpu_entropy=True)
    for f, (y, u, v, _) in enumerate(frames):
        _, rec = hvc.hvc.jpeg_entropy_decode(single[f])
        want = hvc.hvc.jpeg_entropy_encode(info, rec.reshape(-1)[:info.coef_count])
        assert single[f] == batch[f] == batch_gpu[f] == want
        assert want == orc.encode_yuv(y, u, v, w, h, chroma, q)
        assert opt[f] != want


def test_optimised_with_hardcaml_encode_arithmetic(ctx, hvc):
    ctx.set_encode_arithmetic("hardcaml")
    try:
        info, default, opt = check_file_entry_points(ctx, hvc, 96, 64, 420, 80, 9, chunk=4, base=5)
        # the records are the RTL twin's, not the model's
        y, u, v = planes_of(5, 96, 64, 420)
        assert default[0] != orc.encode_yuv(y, u, v, 96, 64, 420, 80)
    finally:
        ctx.set_encode_arithmetic("model")


def test_config5_size_batch_gpu_optimised(ctx, hvc):
    """16 4K 4:2:0 frames through hvc_jpeg_encode_batch_gpu with optimised tables (config 5's frame generator): every
    file equals the host composition of its own record, which the default-table file carries"""
    from video_coding_amd.synth import synth_pixels as synth
    W, H, n = 3840, 2160, 16
    frames = []
    for f in range(n):
        y, u, v = synth(110 + f, H, W), synth(120 + f, H // 2, W // 2), synth(130 + f, H // 2, W // 2)
        frames.append(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]))
    info = hvc.hvc.jpeg_encoder_layout(W, H, 420, 75)
    default, _ = ctx.jpeg_encode_batch(frames, W, H, 420, 75, threads=8, frames_per_chunk=4, gpu_entropy=True)
    ctx.set_huffman_tables("optimised")
    try:
        opt, _ = ctx.jpeg_encode_batch(frames, W, H, 420, 75, threads=8, frames_per_chunk=4, gpu_entropy=True)
    finally:
        ctx.set_huffman_tables("default")
    for f in range(n):
        _, rec = hvc.hvc.jpeg_entropy_decode(default[f])
        rec = np.ascontiguousarray(rec.reshape(-1)[:info.coef_count])
        assert opt[f] == host_file(hvc, info, rec)[1], "frame %d" % f
        assert len(opt[f]) < len(default[f])


def test_set_get_round_trip(ctx, hvc):
    import ctypes as C
    L = hvc.lib()
    assert ctx.huffman_tables == "default"
    ctx.set_huffman_tables("optimised")
    assert ctx.huffman_tables == "optimised"
    for bad in (-1, 2, 7):
        assert L.hvc_set_huffman_tables(ctx._h, bad) == -1
    assert ctx.huffman_tables == "optimised"
    ctx.set_huffman_tables(0)
    v = C.c_int(-5)
    assert L.hvc_get_huffman_tables(ctx._h, C.byref(v)) == 0 and v.value == 0
    assert L.hvc_get_huffman_tables(ctx._h, None) == -1
