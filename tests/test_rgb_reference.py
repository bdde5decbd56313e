"""The definition of "the RGB image of a file" (include/hvc_jpeg.h, RGB; tools/rgb_reference.py) on the CPU: the six
entry points are declared and bound, the numpy definition reproduces libjpeg's two colour steps exactly (libjpeg-turbo
behind PIL: an implementation that shares no code with this repository), its resampling is the checker's, the
properties the header claims hold over all 2^24 inputs, and the command line takes the new flags."""
import io
import os
import re
import sys

import numpy as np
import pytest

from helpers import synth_pixels
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rgb_reference as ref  # noqa: E402

NAMES = ["hvc_yuv_to_rgb", "hvc_rgb_to_yuv", "hvc_decode_frames_rgb", "hvc_jpeg_decode_rgb", "hvc_jpeg_decode_batch_rgb",
         "hvc_jpeg_encode_rgb"]


def test_header_declares_and_binding_lists_the_six_functions():
    import video_coding_amd as hvc
    header = open(os.path.join(ROOT, "include", "hvc_jpeg.h")).read()
    for n in NAMES:
        assert re.search(r"HVC_API int %s\(" % n, header), n
        assert n in hvc.hvc.SYMBOLS, n
    assert re.search(r"HVC_YUV_400 = 400", header)
    assert re.search(r"HVC_RGB_INTERLEAVED = 0, HVC_RGB_PLANAR = 1 \} hvc_rgb_layout;", header)


def test_reference_stands_alone():
    text = open(os.path.join(ROOT, "tools", "rgb_reference.py")).read()
    imports = re.findall(r"^\s*(?:import|from)\s+(\S+)", text, flags=re.M)
    assert imports == ["numpy"], imports


# ---- against libjpeg (through PIL)
def pil_image():
    return pytest.importorskip("PIL.Image")


def libjpeg_ycc(Image, jpeg):
    im = Image.open(io.BytesIO(jpeg))
    im.draft("YCbCr", im.size)
    im.load()
    assert im.mode == "YCbCr"
    return np.asarray(im)


def libjpeg_rgb(Image, jpeg):
    im = Image.open(io.BytesIO(jpeg))
    im.load()
    assert im.mode == "RGB"
    return np.asarray(im)


def test_ycc_to_rgb_is_libjpegs_step_exactly():
    """a 4:4:4 file decoded once to YCbCr and once to RGB: libjpeg's own colour step in isolation"""
    Image = pil_image()
    rng = np.random.Generator(np.random.PCG64(7))
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, size=(256, 256, 3), dtype=np.uint8), "RGB").save(buf, "JPEG", quality=90, subsampling=0)
    ycc, rgb = libjpeg_ycc(Image, buf.getvalue()), libjpeg_rgb(Image, buf.getvalue())
    assert len(np.unique(ycc.reshape(-1, 3), axis=0)) > 30000
    got = np.stack(ref.ycc_to_rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2]), axis=2)
    assert int((got != rgb).sum()) == 0
    assert np.array_equal(ref.planes_to_rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2], 444, 256, 256), rgb)


def test_rgb_to_ycc_is_libjpegs_step_exactly():
    """32 x 32 flat 8 x 8 blocks at quality 100, 4:4:4: flat blocks survive a table of ones, so the planes libjpeg hands
    back are its RGB -> YCbCr step"""
    Image = pil_image()
    rng = np.random.Generator(np.random.PCG64(8))
    colours = rng.integers(0, 256, size=(32, 32, 3), dtype=np.uint8)
    colours[0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 0, 255]]
    image = np.repeat(np.repeat(colours, 8, axis=0), 8, axis=1)
    buf = io.BytesIO()
    Image.fromarray(image, "RGB").save(buf, "JPEG", quality=100, subsampling=0)
    ycc = libjpeg_ycc(Image, buf.getvalue())
    y, cb, cr = ref.rgb_to_planes(image, 444)
    assert int((np.stack([y, cb, cr], axis=2) != ycc).sum()) == 0


@pytest.mark.parametrize("w,h,q", [(64, 48, 75), (200, 120, 95), (96, 64, 30)])
def test_whole_444_files_within_three_of_libjpeg(w, h, q):
    """the three 4:4:4 cases of tests/test_third_party_crosscheck.py: that file pins the planes within 1 of libjpeg's, and
    one step of Y moves a channel by 1, one step of Cb or Cr moves each rounded chroma term by at most 2 (116130 / 65536
    < 2; G: (22554 + 46802) / 65536 < 2): at most 3 per channel"""
    Image = pil_image()
    r8 = lambda x: (x + 7) // 8 * 8
    planes = [synth_pixels(40 + i, r8(h), r8(w))[:h, :w] for i in range(3)]
    jpeg = orc.encode_yuv(planes[0], planes[1], planes[2], w, h, 444, q)
    d = orc.Decoder(jpeg)
    d.decode()
    got = ref.planes_to_rgb(d.plane(0), d.plane(1), d.plane(2), 444, w, h).astype(np.int64)
    want = libjpeg_rgb(Image, jpeg).astype(np.int64)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 3


# ---- the resampling is the checker's
@pytest.mark.parametrize("cw,ch", [(1, 1), (2, 3), (9, 5), (27, 23), (64, 8)])
def test_resampling_equals_the_checkers(cw, ch):
    rng = np.random.Generator(np.random.PCG64(cw * 100 + ch))
    src = rng.integers(0, 256, size=(ch, cw), dtype=np.uint8)
    assert np.array_equal(ref.supersample_hv2(src), orc.supersample_hv2(src))
    assert np.array_equal(ref.supersample_h2(src), orc.supersample_h2(src))
    big = rng.integers(0, 256, size=(2 * ch, 2 * cw), dtype=np.uint8)
    assert np.array_equal(ref.subsample_hv2(big), orc.subsample_hv2(big, cw, ch))
    assert np.array_equal(ref.subsample_h2(big), orc.subsample_h2(big, cw, 2 * ch))


@pytest.mark.parametrize("sampling", [420, 422, 444, 400])
@pytest.mark.parametrize("w,h", [(1, 1), (3, 3), (17, 9), (18, 10), (53, 45)])
def test_odd_sizes_use_the_ceil_window_of_the_decoded_plane(sampling, w, h):
    """stage 2 for any size: the cw x ch window is supersampled by the checker and cut to width x height; what lies in the
    decoded planes beyond the window does not matter"""
    rng = np.random.Generator(np.random.PCG64(w * 1000 + h))
    cw, ch = ref.chroma_window(sampling, w, h)
    planes = [rng.integers(0, 256, size=(h + 16, w + 16), dtype=np.uint8) for _ in range(3)]
    got = ref.planes_to_rgb(planes[0], planes[1], planes[2], sampling, w, h)
    if sampling == 400:
        want = np.stack([planes[0][:h, :w]] * 3, axis=2)
    else:
        up = {420: orc.supersample_hv2, 422: orc.supersample_h2, 444: lambda p: p}[sampling]
        full = [up(np.ascontiguousarray(p[:ch, :cw]))[:h, :w] for p in planes[1:]]
        want = np.stack(ref.ycc_to_rgb(planes[0][:h, :w], full[0], full[1]), axis=2)
    assert np.array_equal(got, want)
    noisy = [p.copy() for p in planes]
    for p in noisy[1:]:
        p[ch:, :] ^= 0xff
        p[:, cw:] ^= 0xff
    assert np.array_equal(ref.planes_to_rgb(noisy[0], noisy[1], noisy[2], sampling, w, h), got)
    assert np.array_equal(ref.planes_to_rgb(planes[0], planes[1], planes[2], sampling, w, h, "planar"), got.transpose(2, 0, 1))


def test_encode_direction_keeps_the_encoders_rule():
    image = np.zeros((3, 3, 3), dtype=np.uint8)
    for sampling in (420, 422):
        with pytest.raises(ValueError):
            ref.rgb_to_planes(image, sampling)
    with pytest.raises(ValueError):
        ref.rgb_to_planes(image[:, :2], 420)
    assert ref.rgb_to_planes(image[:, :2], 422)[1].shape == (3, 1)
    assert ref.rgb_to_planes(image, 444)[1].shape == (3, 3)
    assert ref.rgb_to_planes(image, 400)[1] is None


# ---- properties over all 2^24 inputs
def all_triples():
    v = np.arange(1 << 24, dtype=np.int64)
    return v >> 16, (v >> 8) & 255, v & 255


def test_forward_outputs_need_no_clamp():
    y, cb, cr = ref.rgb_to_ycc_unclamped(*all_triples())
    for c in (y, cb, cr):
        assert int(c.min()) >= 0 and int(c.max()) <= 255


def test_grey_maps_to_grey_and_back():
    v = np.arange(256, dtype=np.uint8)
    y, cb, cr = ref.rgb_to_ycc(v, v, v)
    assert np.array_equal(y, v) and (cb == 128).all() and (cr == 128).all()
    r, g, b = ref.ycc_to_rgb(y, cb, cr)
    assert np.array_equal(r, v) and np.array_equal(g, v) and np.array_equal(b, v)


def test_round_trip_within_one():
    r, g, b = all_triples()
    back = ref.ycc_to_rgb(*ref.rgb_to_ycc(r, g, b))
    for a, c in zip((r, g, b), back):
        assert int(np.abs(a - c.astype(np.int64)).max()) <= 1


# ---- the command line
def test_cli_takes_the_new_flags():
    import video_coding_amd.__main__ as cli
    a = cli.parser().parse_args("model decode frame in.jpg out.ppm -rgb -restart-markers".split())
    assert a.rgb and a.restart_markers and a.yuv == "out.ppm" and a.fn is cli.model_decode_frame
    a = cli.parser().parse_args("model encode frame in.ppm 64x48 out.jpg -rgb -chroma 444 -huffman optimised -restart-interval 4".split())
    assert a.rgb and a.size == (64, 48) and a.chroma == 444 and a.huffman == "optimised" and a.restart_interval == 4
    assert not cli.parser().parse_args("model decode frame in.jpg".split()).rgb
    assert not cli.parser().parse_args("model encode frame in.yuv 64x48 out.jpg".split()).rgb


def test_cli_refuses_a_ppm_of_another_size_before_any_gpu_call(tmp_path, monkeypatch):
    import video_coding_amd.__main__ as cli
    ppm = tmp_path / "in.ppm"
    image = np.arange(6 * 4 * 3, dtype=np.uint8).reshape(4, 6, 3)
    ref.write_ppm(str(ppm), image)
    assert np.array_equal(cli.read_ppm(str(ppm), (6, 4)), image)

    def no_gpu(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(cli.hvc, "Context", no_gpu)
    with pytest.raises(SystemExit) as e:
        cli.main(["model", "encode", "frame", str(ppm), "8x4", str(tmp_path / "out.jpg"), "-rgb"])
    assert "6x4" in str(e.value) and "8x4" in str(e.value)
    assert not (tmp_path / "out.jpg").exists()
    (tmp_path / "bad.ppm").write_bytes(b"P5\n6 4\n255\n" + bytes(24))
    with pytest.raises(SystemExit):
        cli.main(["model", "encode", "frame", str(tmp_path / "bad.ppm"), "6x4", str(tmp_path / "out.jpg"), "-rgb"])
