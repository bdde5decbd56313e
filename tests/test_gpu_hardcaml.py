"""The Hardcaml RTL twin on the GPU (hvc_set_arithmetic HVC_ARITH_HARDCAML, k_hardcaml): bit for bit the numpy restatement
of tests/test_hardcaml_twin.py on every routed entry point, the reference's RTL vectors, the divergence call, isolation
of the setting, and `simulate decoder`."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden_bytes
from helpers import synth_coefs
from oracle import orc
from test_hardcaml_twin import G9, ROM, hardcaml_blocks, sext
from test_gpu_model_corners import wide_dc_file_420

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


def fresh():
    import video_coding_amd as hvc
    return hvc.Context(0)


def restate_record(info, coefs):
    """the RTL's padded pixel record of one frame from its coefficient record"""
    out = np.zeros(info.pixel_bytes, dtype=np.uint8)
    q = info.qtab_array()
    for k in range(info.n_comp):
        L = info.layout[k]
        bw, bh = L.blocks_w, L.blocks_h
        blk = coefs[L.coef_offset:L.coef_offset + bw * bh * 64].reshape(bh, bw, 64)
        px = hardcaml_blocks(blk, q[L.qtab]).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        plane = out[L.plane_offset:L.plane_offset + L.stride * bh * 8].reshape(bh * 8, L.stride)
        plane[:, :bw * 8] = px
    return out


def plane_of(blocks_px, bw, bh):
    return blocks_px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def decode_plane(ctx, coefs, q, bw, bh):
    out = np.zeros((bh * 8, bw * 8), dtype=np.uint8)
    ctx.dequant_idct_recon(np.ascontiguousarray(coefs, dtype=np.int16), q, bw, bh, 1, out)
    return out


def test_mouse480_blocks_equal_the_rtl_fixture(ctx):
    import video_coding_amd as hvc
    data = golden_bytes("Mouse480.jpg")
    ctx.set_arithmetic("hardcaml")
    try:
        info, pixels = ctx.jpeg_decode(data)
    finally:
        ctx.set_arithmetic("model")
    _, coefs = hvc.hvc.jpeg_entropy_decode(data)
    pos = hvc.hvc.decode_order_positions(info)
    planes = info.planes(pixels)
    ends = np.cumsum([info.layout[k].blocks_w * info.layout[k].blocks_h for k in range(info.n_comp)])
    for want in G9["mouse_blocks"]:
        p = int(pos[want["block_number"]])
        k = int(np.searchsorted(ends, p, side="right"))
        b = p - (int(ends[k - 1]) if k else 0)
        bw = info.layout[k].blocks_w
        blk = planes[k][(b // bw) * 8:(b // bw) * 8 + 8, (b % bw) * 8:(b % bw) * 8 + 8]
        assert blk.reshape(-1).tolist() == want["pixels"], want["block_number"]
    specs = [dict(blocks_w=L.blocks_w, blocks_h=L.blocks_h, qtab=L.qtab, coef_offset=L.coef_offset) for L in info.layout[:info.n_comp]]
    div = ctx.decode_divergence(coefs, info.coef_count, info.qtab_array(), specs, 1)[0]
    assert div[pos[:6]].tolist() == [m["max_reconstructed_diff"] for m in G9["mouse_blocks"]]
    assert np.array_equal(pixels, restate_record(info, coefs))


def test_idct_vector_through_a_one_block_record(ctx):
    v = G9["idct"]
    X = np.array(v["dct_inputs"]).reshape(8, 8).reshape(-1)
    from test_hardcaml_twin import ZI
    rec = np.zeros(64, dtype=np.int16)
    rec[:] = X[ZI]   # zig-zag record whose natural placement is the vector
    ctx.set_arithmetic("hardcaml")
    try:
        out = decode_plane(ctx, rec, np.ones(64, np.uint16), 1, 1)
    finally:
        ctx.set_arithmetic("model")
    assert (out.astype(np.int64) - 128).reshape(-1).tolist() == v["pixels"]


def tables():
    rng = np.random.default_rng(3)
    yield np.ones(64, np.uint16)
    yield rng.integers(0, 256, 64).astype(np.uint16)
    q = rng.integers(0, 65536, 64).astype(np.uint16)
    q[:4] = [0, 1, 255, 256]
    q[4:8] = [257, 511, 4095, 65535]
    yield q
    yield (orc.quant_scale(orc.quant_luma(), 75)).astype(np.uint16)


@pytest.mark.parametrize("qi", range(4))
def test_random_full_range_records(ctx, qi):
    q = list(tables())[qi]
    rng = np.random.default_rng(100 + qi)
    bw, bh = 37, 11
    coefs = rng.integers(-32768, 32768, (bh * bw, 64)).astype(np.int16)
    coefs[::3] = (coefs[::3] % 64) - 32   # small values too
    ctx.set_arithmetic("hardcaml")
    try:
        got = decode_plane(ctx, coefs, q, bw, bh)
    finally:
        ctx.set_arithmetic("model")
    assert np.array_equal(got, plane_of(hardcaml_blocks(coefs, q), bw, bh))


def test_worst_case_blocks_reach_the_int32_bound(ctx):
    """blocks whose 12-bit inputs follow the signs of the ROM: the largest |T| and |R| any input produces"""
    from test_hardcaml_twin import ZI, dequant_rtl, idct_rtl
    recs = []
    for r in range(8):
        for y in range(8):
            for s in (1, -1):
                X = np.zeros((8, 8), dtype=np.int64)
                X[:, y] = np.where(ROM[r] * s >= 0, 2047, -2048)
                rec = np.zeros(64, dtype=np.int64)
                rec[:] = X.reshape(-1)[ZI]
                recs.append(rec)
                # all columns alike: pass 2 sees the largest T in a whole row
                X2 = np.repeat(np.where(ROM[r] * s >= 0, 2047, -2048)[:, None], 8, axis=1)
                rec2 = np.zeros(64, dtype=np.int64)
                rec2[:] = X2.reshape(-1)[ZI]
                recs.append(rec2)
    coefs = np.array(recs).astype(np.int16)
    T, _ = idct_rtl(dequant_rtl(coefs, np.ones(64)))
    assert int(np.abs(T).max()) >= 86000
    bw = coefs.shape[0]
    ctx.set_arithmetic("hardcaml")
    try:
        got = decode_plane(ctx, coefs, np.ones(64, np.uint16), bw, 1)
    finally:
        ctx.set_arithmetic("model")
    assert np.array_equal(got, plane_of(hardcaml_blocks(coefs, np.ones(64)), bw, 1))


def test_exhaustive_position_by_value(ctx):
    """every zig-zag position x every 12-bit value, q = 1 (the product then is the value itself)"""
    vals = np.arange(-2048, 2048, dtype=np.int64)
    coefs = np.zeros((64, 4096, 64), dtype=np.int16)
    for z in range(64):
        coefs[z, :, z] = vals
    coefs = coefs.reshape(64 * 4096, 64)
    bw, bh = 512, 512
    ctx.set_arithmetic("hardcaml")
    try:
        got = decode_plane(ctx, coefs, np.ones(64, np.uint16), bw, bh)
    finally:
        ctx.set_arithmetic("model")
    assert np.array_equal(got, plane_of(hardcaml_blocks(coefs, np.ones(64)), bw, bh))


def _big_file():
    y = np.asarray(np.random.default_rng(1).integers(0, 256, (480, 640)), dtype=np.uint8)
    u = np.asarray(np.random.default_rng(2).integers(0, 256, (240, 320)), dtype=np.uint8)
    v = np.asarray(np.random.default_rng(3).integers(0, 256, (240, 320)), dtype=np.uint8)
    return orc.encode_yuv(y, u, v, 640, 480, 420, 90)


def test_every_routed_entry_point(ctx):
    import torch
    import video_coding_amd as hvc
    files = [golden_bytes("Mouse480.jpg"), golden_bytes("mini.jpg"), _big_file()]
    assert len(files[2]) >= 128 * 1024   # the single-file GPU reader takes it
    c = fresh()
    try:
        c.set_arithmetic("hardcaml")
        for data in files:
            info, coefs = hvc.hvc.jpeg_entropy_decode(data)
            want = restate_record(info, coefs)
            _, px = c.jpeg_decode(data)
            assert np.array_equal(px, want)
            specs = [dict(blocks_w=L.blocks_w, blocks_h=L.blocks_h, qtab=L.qtab, coef_offset=L.coef_offset,
                          plane_offset=L.plane_offset, stride=L.stride) for L in info.layout[:info.n_comp]]
            q = info.qtab_array()
            # host memory, two frames
            two = np.concatenate([coefs, coefs])
            out = np.zeros(2 * info.pixel_bytes, np.uint8)
            c.decode_frames(two, info.coef_count, q, specs, 2, out, info.pixel_bytes)
            assert np.array_equal(out, np.concatenate([want, want]))
            # device memory
            d_c = torch.from_numpy(two).cuda()
            d_p = torch.zeros(2 * info.pixel_bytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c.decode_frames(d_c, info.coef_count, q, specs, 2, d_p, info.pixel_bytes)
            c.synchronize()
            assert np.array_equal(d_p.cpu().numpy(), np.concatenate([want, want]))
            # the asynchronous seam
            pin_c, pin_p = c.host_alloc(coefs.shape, np.int16), c.host_alloc((info.pixel_bytes,), np.uint8)
            pin_c[:] = coefs
            pin_p[:] = 0
            c.decode_frames_submit(0, pin_c, info.coef_count, q, specs, 1, pin_p, info.pixel_bytes)
            c.wait(0)
            assert np.array_equal(pin_p, want)
            c.host_free(pin_c)
            c.host_free(pin_p)
            # both batch pipelines, host and device output
            batch = [data] * 5
            for gpu in (False, True):
                o = np.zeros(5 * info.pixel_bytes, np.uint8)
                c.jpeg_decode_batch(batch, o, info.pixel_bytes, threads=2, frames_per_chunk=2, gpu_entropy=gpu)
                assert np.array_equal(o.reshape(5, -1), np.tile(want, (5, 1))), gpu
                od = torch.zeros(5 * info.pixel_bytes, dtype=torch.uint8, device="cuda")
                c.jpeg_decode_batch(batch, od, info.pixel_bytes, threads=2, frames_per_chunk=3, gpu_entropy=gpu)
                assert np.array_equal(od.cpu().numpy().reshape(5, -1), np.tile(want, (5, 1))), gpu
        assert c.last_wide_blocks() == 0
    finally:
        c.close()


def test_wide_dc_file(ctx):
    """a file whose absolute DCs leave int16: the record holds them saturated, the side list the true value, of which the
    RTL keeps the low 12 bits"""
    import video_coding_amd as hvc
    data = wide_dc_file_420([20, 33, 11, 62, 47, 3], 72, 40, 97, 7)
    info = hvc.hvc.jpeg_read_header(data)
    rec = orc.Decoder(data).coef_record()
    coefs = np.array([int(v) & 0xFFF for v in np.asarray(rec).reshape(-1)], dtype=np.int64)
    want = restate_record(info, sext(coefs, 12))
    c = fresh()
    try:
        c.set_arithmetic("hardcaml")
        _, px = c.jpeg_decode(data)
        assert np.array_equal(px, want)
        o = np.zeros(3 * info.pixel_bytes, np.uint8)
        c.jpeg_decode_batch([data] * 3, o, info.pixel_bytes, threads=2, frames_per_chunk=2)
        assert np.array_equal(o.reshape(3, -1), np.tile(want, (3, 1)))
    finally:
        c.close()


def test_isolation_and_the_444_refusal():
    import video_coding_amd as hvc
    data = golden_bytes("Mouse480.jpg")
    a, b = fresh(), fresh()
    try:
        assert a.arithmetic == "model" and b.arithmetic == "model"
        _, ref = b.jpeg_decode(data)
        a.set_arithmetic("hardcaml")
        assert a.arithmetic == "hardcaml"
        _, hc = a.jpeg_decode(data)
        assert not np.array_equal(hc, ref)
        _, again = b.jpeg_decode(data)   # a second context is unaffected
        assert np.array_equal(again, ref)
        with pytest.raises(hvc.HvcError) as e:
            a.set_arithmetic(2)
        assert e.value.code == -1 and a.arithmetic == "hardcaml"
        # the fused 4:4:4 entry points refuse and leave their output untouched
        with pytest.raises(hvc.HvcError):
            a.jpeg_decode_yuv444(data)
        info, coefs = hvc.hvc.jpeg_entropy_decode(data)
        specs = [dict(blocks_w=L.blocks_w, blocks_h=L.blocks_h, qtab=L.qtab, coef_offset=L.coef_offset) for L in info.layout[:3]]
        frames = np.full(3 * info.width * info.height, 7, np.uint8)
        with pytest.raises(hvc.HvcError) as e:
            a.decode_frames_yuv444(coefs, info.coef_count, info.qtab_array(), specs, 1, info.width, info.height, frames)
        assert e.value.code == -1 and (frames == 7).all()
        for gpu in (False, True):
            with pytest.raises(hvc.HvcError) as e:
                a.jpeg_decode_batch([data] * 2, frames, 0, threads=1, frames_per_chunk=1, yuv444=True, gpu_entropy=gpu)
            assert e.value.code == -1 and (frames == 7).all()
        a.set_arithmetic("model")
        _, back = a.jpeg_decode(data)
        assert np.array_equal(back, ref)
        # the encoder ignores the setting
        a.set_arithmetic("hardcaml")
        y, u, v = orc.split_yuv(golden_bytes("mini64x64.420"), 64, 64, 420)
        assert a.jpeg_encode(y, u, v, 64, 64, 420, 75) == golden_bytes("mini.jpg")
    finally:
        a.close()
        b.close()


def test_divergence_on_random_records_and_photo_content(ctx):
    import torch
    q = orc.quant_scale(orc.quant_luma(), 50).astype(np.uint16)
    bw, bh = 45, 13
    coefs, _ = synth_coefs(77, bh, bw, q)
    rng = np.random.default_rng(5)
    coefs = coefs.reshape(-1, 64).copy()
    coefs[::4] = rng.integers(-2048, 2048, (coefs[::4].shape)).astype(np.int16)
    model = orc.dequant_idct_recon(coefs.reshape(-1), q, bw, bh).reshape(bh * 8, bw * 8)
    hc = plane_of(hardcaml_blocks(coefs, q), bw, bh)
    want = np.abs(model.astype(np.int64) - hc).reshape(bh, 8, bw, 8).max(axis=(1, 3)).reshape(-1)
    specs = [dict(blocks_w=bw, blocks_h=bh, qtab=0, coef_offset=0)]
    for arith in ("model", "hardcaml"):   # independent of the setting
        ctx.set_arithmetic(arith)
        got = ctx.decode_divergence(coefs.reshape(-1), bw * bh * 64, q, specs, 1)[0]
        assert np.array_equal(got, want), arith
    ctx.set_arithmetic("model")
    # two frames in device memory, a padded diff stride
    d_c = torch.from_numpy(np.concatenate([coefs.reshape(-1)] * 2)).cuda()
    d_d = torch.full((2 * (bw * bh + 16),), 255, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_divergence(d_c, bw * bh * 64, q, specs, 2, d_d, bw * bh + 16)
    ctx.synchronize()
    dd = d_d.cpu().numpy().reshape(2, -1)
    assert np.array_equal(dd[:, :bw * bh], np.stack([want, want])) and (dd[:, bw * bh:] == 255).all()
    # photo-like content: the Mouse480 frame
    import video_coding_amd as hvc
    data = golden_bytes("Mouse480.jpg")
    info, co = hvc.hvc.jpeg_entropy_decode(data)
    d = orc.Decoder(data)
    d.decode()
    hcrec = restate_record(info, co)
    wants = []
    for k in range(3):
        L = info.layout[k]
        m = d.plane(k).astype(np.int64)
        h = info.planes(hcrec)[k].astype(np.int64)
        wants.append(np.abs(m - h).reshape(L.blocks_h, 8, L.blocks_w, 8).max(axis=(1, 3)).reshape(-1))
    specs = [dict(blocks_w=L.blocks_w, blocks_h=L.blocks_h, qtab=L.qtab, coef_offset=L.coef_offset) for L in info.layout[:3]]
    got = ctx.decode_divergence(co, info.coef_count, info.qtab_array(), specs, 1)[0]
    assert np.array_equal(got, np.concatenate(wants))
    assert got.max() <= 2   # the reference's tolerance holds on this file


def test_simulate_decoder_cli(tmp_path):
    import video_coding_amd as hvc
    src = os.path.join(ROOT, "tests", "golden", "Mouse480.jpg")
    out = tmp_path / "out.yuv"
    r = subprocess.run([sys.executable, "-m", "video_coding_amd", "simulate", "decoder", src, "-yuv", str(out), "-blocks", "6",
                        "-error-tolerance", "0"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    recs = []
    for line in r.stdout.splitlines():
        m = re.match(r"\(\(block_number (\d+)\) \(max_reconstructed_diff (\d+)\) \(pixels \((.*)\)\)\)$", line)
        assert m, line
        recs.append({"block_number": int(m.group(1)), "max_reconstructed_diff": int(m.group(2)),
                     "pixels": [int(v, 16) for v in re.findall(r"[0-9a-f]{2}", m.group(3))]})
    assert recs == G9["mouse_blocks"]
    data = golden_bytes("Mouse480.jpg")
    info, coefs = hvc.hvc.jpeg_entropy_decode(data)
    frame = hvc.hvc.jpeg_get_yuv_frame(info, restate_record(info, coefs))
    assert out.read_bytes() == frame.tobytes() and len(frame) == 480 * 320 * 3 // 2
