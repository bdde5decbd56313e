"""The profiling ring (hvc_set_profiling / hvc_kernel_ms_history): which calls take an entry of it, that every call leaves
the setting as it found it, and that the divergence calls leave the arithmetic settings alone.

The probe needs nothing beyond the ABI: hvc_kernel_ms_history(n) is HVC_E_INVALID_ARG exactly when n exceeds the number of
entries taken since hvc_set_profiling, so "entries taken" is the largest n that succeeds."""
import numpy as np
import pytest

from conftest import golden_bytes
from test_hardcaml_encoder_twin import hardcaml_encode_blocks
from test_hardcaml_twin import hardcaml_blocks

pytestmark = pytest.mark.gpu

E_INVALID_ARG = -1
PROBE_MAX = 8

# 2 frames of one 3 x 2-block component: a partial 64-block tile
BW, BH, NF = 3, 2, 2
SPEC = [dict(blocks_w=BW, blocks_h=BH, qtab=0, coef_offset=0, plane_offset=0, stride=BW * 8)]
REC = BW * BH * 64
# a 16 x 16 4:2:0 frame: luma 2 x 2 blocks, chroma 1 x 1
SPEC420 = [dict(blocks_w=2, blocks_h=2, qtab=0, coef_offset=0, plane_offset=0, stride=16),
           dict(blocks_w=1, blocks_h=1, qtab=1, coef_offset=256, plane_offset=256, stride=8),
           dict(blocks_w=1, blocks_h=1, qtab=1, coef_offset=320, plane_offset=320, stride=8)]
REC420 = 384


@pytest.fixture(scope="module")
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(7)
    q = rng.integers(1, 256, (2, 64)).astype(np.uint16)   # every entry at or below 255
    q16 = q.copy()
    q16[1, 5] = 300                                       # one above: the all-int64 kernel
    return dict(q=q, q16=q16,
                coefs=rng.integers(-60, 61, (NF, REC)).astype(np.int16),
                pixels=rng.integers(0, 256, (NF, REC)).astype(np.uint8),
                coefs420=rng.integers(-60, 61, (1, REC420)).astype(np.int16))


def taken(ctx):
    """entries of the ring taken since set_profiling"""
    import video_coding_amd as hvc
    n = 0
    for k in range(1, PROBE_MAX + 1):
        try:
            ctx.kernel_ms_history(k)
        except hvc.hvc.HvcError as e:
            assert e.code == E_INVALID_ARG
            break
        n = k
    return n


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def place(a, device):
    return dev(a) if device else np.ascontiguousarray(a).copy()


def decode_device(ctx, data):
    px = dev(np.zeros((NF, REC), np.uint8))
    ctx.decode_frames(dev(data["coefs"]), REC, data["q"][:1], SPEC, NF, px, REC)
    ctx.synchronize()
    return px.cpu().numpy()


# ---- the calls: name -> f(ctx, data, device)
def c_decode_frames(ctx, d, device):
    ctx.decode_frames(place(d["coefs"], device), REC, d["q"][:1], SPEC, NF, place(np.zeros((NF, REC), np.uint8), device), REC)


def c_encode_frames(ctx, d, device):
    ctx.encode_frames(place(d["pixels"], device), REC, d["q"][:1], SPEC, NF, place(np.zeros((NF, REC), np.int16), device), REC)


def c_dequant_idct_recon(ctx, d, device):
    ctx.dequant_idct_recon(place(d["coefs"], device), d["q"][0], BW, BH, NF, place(np.zeros((NF, REC), np.uint8), device))


def c_fdct_quant(ctx, d, device):
    ctx.fdct_quant(place(d["pixels"], device), d["q"][0], BW, BH, NF, place(np.zeros((NF, REC), np.int16), device))


def c_decode_frames_yuv444(ctx, d, device, q="q"):
    ctx.decode_frames_yuv444(place(d["coefs420"], device), REC420, d[q], SPEC420, 1, 16, 16, place(np.zeros(3 * 256, np.uint8), device))


def c_decode_frames_yuv444_wide(ctx, d, device):
    c_decode_frames_yuv444(ctx, d, device, q="q16")


def c_decode_frames_rgb(ctx, d, device):
    ctx.decode_frames_rgb(place(d["coefs420"], device), REC420, d["q"], SPEC420, 420, 1, 16, 16, place(np.zeros(3 * 256, np.uint8), device))


def c_decode_divergence(ctx, d, device):
    ctx.decode_divergence(place(d["coefs"], device), REC, d["q"][:1], SPEC, NF, place(np.zeros((NF, BW * BH), np.uint8), device), BW * BH)


def c_encode_divergence(ctx, d, device):
    ctx.encode_divergence(place(d["pixels"], device), REC, d["q"][:1], SPEC, NF, place(np.zeros((NF, BW * BH), np.uint8), device), BW * BH)


def c_encode_frames_recon(ctx, d, device):
    z = lambda dt: place(np.zeros((NF, REC), dt), device)
    ctx.encode_frames_recon(place(d["pixels"], device), REC, d["q"][:1], SPEC, NF, z(np.int16), REC, z(np.uint8), z(np.uint8))


def c_submit_wait(ctx, d, device):
    pin_c, pin_p = ctx.host_alloc((NF, REC), np.int16), ctx.host_alloc((NF, REC), np.uint8)
    pin_c[:] = d["coefs"]
    try:
        ctx.decode_frames_submit(0, pin_c, REC, d["q"][:1], SPEC, NF, pin_p, REC)
        ctx.wait(0)
    finally:
        ctx.host_free(pin_c)
        ctx.host_free(pin_p)


def _mini_planes():
    from oracle import orc
    return orc.split_yuv(golden_bytes("mini64x64.420"), 64, 64, 420)


def c_jpeg_decode(ctx, d, device):
    ctx.jpeg_decode(golden_bytes("mini.jpg"))


def c_jpeg_decode_yuv444(ctx, d, device):
    ctx.jpeg_decode_yuv444(golden_bytes("mini.jpg"))


def c_jpeg_decode_rgb(ctx, d, device):
    ctx.jpeg_decode_rgb(golden_bytes("mini.jpg"))


def c_jpeg_encode(ctx, d, device):
    y, u, v = _mini_planes()
    ctx.jpeg_encode(y, u, v, 64, 64, 420, 75)


def _batch(ctx, device, gpu_entropy):
    import video_coding_amd as hvc
    mini = golden_bytes("mini.jpg")
    fs = hvc.hvc.jpeg_read_header(mini).pixel_bytes
    ctx.jpeg_decode_batch([mini, mini], place(np.zeros((2, fs), np.uint8), device), fs, threads=2, frames_per_chunk=2,
                          gpu_entropy=gpu_entropy)


def c_jpeg_decode_batch(ctx, d, device):
    _batch(ctx, device, False)


def c_jpeg_decode_batch_gpu(ctx, d, device):
    _batch(ctx, device, True)


DEVICE, HOST = True, False
CASES = [
    # a device-memory call of the block stage takes one entry ...
    (c_decode_frames, DEVICE, 1), (c_encode_frames, DEVICE, 1), (c_dequant_idct_recon, DEVICE, 1), (c_fdct_quant, DEVICE, 1),
    (c_decode_frames_yuv444, DEVICE, 1), (c_decode_frames_rgb, DEVICE, 1),
    # ... but not the fused call that goes through the all-int64 kernel, and no host-memory call
    (c_decode_frames_yuv444_wide, DEVICE, 0),
    (c_decode_frames, HOST, 0), (c_encode_frames, HOST, 0), (c_dequant_idct_recon, HOST, 0), (c_fdct_quant, HOST, 0),
    (c_decode_frames_yuv444, HOST, 0),
    # (hvc_decode_frames_rgb stages host records itself and runs the device-memory block stage on them, with profiling as the
    # context has it: one entry per part, as in the parent commit)
    (c_decode_frames_rgb, HOST, 1),
    # callers of the block stage that keep their launches out of the ring
    (c_decode_divergence, DEVICE, 0), (c_decode_divergence, HOST, 0), (c_encode_divergence, DEVICE, 0), (c_encode_divergence, HOST, 0),
    (c_encode_frames_recon, DEVICE, 0), (c_encode_frames_recon, HOST, 0), (c_submit_wait, HOST, 0),
    # the file-level calls (mini.jpg; the batch calls on 2 copies of it): these figures were taken from the parent commit
    (c_jpeg_decode, HOST, 0), (c_jpeg_decode_yuv444, HOST, 0), (c_jpeg_decode_rgb, HOST, 0), (c_jpeg_encode, HOST, 0),
    (c_jpeg_decode_batch, HOST, 0), (c_jpeg_decode_batch, DEVICE, 0), (c_jpeg_decode_batch_gpu, HOST, 0), (c_jpeg_decode_batch_gpu, DEVICE, 0),
]


@pytest.mark.parametrize("call,device,entries", CASES, ids=["%s-%s" % (f.__name__[2:], "device" if dv else "host") for f, dv, _ in CASES])
def test_entries_taken_and_the_setting_survives(ctx, data, call, device, entries):
    ctx.set_profiling(True)
    assert taken(ctx) == 0   # set_profiling starts the count over (the cases before this one took entries)
    call(ctx, data, device)
    ctx.synchronize()
    print("%s %s: %d entries" % (call.__name__[2:], "device" if device else "host", taken(ctx)))
    assert taken(ctx) == entries
    decode_device(ctx, data)   # the setting is still on: exactly one more
    assert taken(ctx) == entries + 1
    ctx.set_profiling(False)
    decode_device(ctx, data)
    assert taken(ctx) == 0


def test_set_profiling_starts_the_count_over(ctx, data):
    ctx.set_profiling(True)
    for k in range(3):
        decode_device(ctx, data)
        assert taken(ctx) == k + 1
    ctx.set_profiling(True)
    assert taken(ctx) == 0
    ctx.set_profiling(False)


@pytest.mark.parametrize("device", [True, False])
def test_divergence_calls_leave_the_arithmetic_settings_alone(ctx, data, device):
    q = data["q"][0]
    want_px = hardcaml_blocks(data["coefs"].reshape(NF, BH, BW, 64), q)                   # [NF, BH, BW, 8, 8]
    want_px = want_px.transpose(0, 1, 3, 2, 4).reshape(NF, REC)
    blocks = data["pixels"].reshape(NF, BH, 8, BW, 8).transpose(0, 1, 3, 2, 4).reshape(-1, 8, 8)
    want_co = hardcaml_encode_blocks(blocks, q).reshape(NF, REC)
    ctx.set_arithmetic("hardcaml")
    ctx.set_encode_arithmetic("hardcaml")
    try:
        for div in (c_decode_divergence, c_encode_divergence):
            div(ctx, data, device)
            assert ctx.arithmetic == "hardcaml" and ctx.encode_arithmetic == "hardcaml"
            assert np.array_equal(decode_device(ctx, data), want_px)
            co = dev(np.zeros((NF, REC), np.int16))
            ctx.encode_frames(dev(data["pixels"]), REC, data["q"][:1], SPEC, NF, co, REC)
            ctx.synchronize()
            assert np.array_equal(co.cpu().numpy(), want_co)
    finally:
        ctx.set_arithmetic("model")
        ctx.set_encode_arithmetic("model")
