"""tools/libjpeg_reference.py -- the numpy statement of include/hvc_jpeg.h, "Bit-exact to libjpeg" (islow inverse DCT,
fancy upsampling, the colour matrix) -- against libjpeg-turbo through Pillow: 0 mismatching bytes on the golden files, on
Pillow-written files and on files written by tools/jpeg_opt_writer.py from random records.  Beside it, on the CPU: the
pins of tests/golden/libjpeg_pins.json, the header, the binding and the command line.  The coefficients of a file come from
the library's host reader (hvc_jpeg_entropy_decode: no GPU), the decode from numpy alone."""
import io
import json
import os
import re
import sys

import numpy as np
import pytest

import libjpeg_files as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import libjpeg_reference as lj  # noqa: E402


def pil():
    return pytest.importorskip("PIL.Image")


def pillow_rgb(data):
    im = pil().open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


def pillow_ycc(data):
    im = pil().open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    im.load()
    assert im.mode == "YCbCr"
    return np.asarray(im)


def reference_rgb(data):
    """a file's RGB image by the definition"""
    from video_coding_amd import hvc
    info, coefs = hvc.jpeg_entropy_decode(data)
    return lj.record_to_rgb(coefs, info.qtab_array(), lf.planes_of_info(info), lf.sampling_of_info(info), info.width, info.height)


def reference_planes(data):
    from video_coding_amd import hvc
    info, coefs = hvc.jpeg_entropy_decode(data)
    return info, lj.record_planes(coefs, info.qtab_array(), lf.planes_of_info(info))


def mismatches(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return int(np.count_nonzero(a != b))


# ---- the reference stands alone
def test_reference_stands_alone():
    text = open(os.path.join(ROOT, "tools", "libjpeg_reference.py")).read()
    imports = re.findall(r"^\s*(?:import|from)\s+(\S+)", text, flags=re.M)
    assert sorted(imports) == ["numpy", "os", "re"], imports


# ---- golden files
@pytest.mark.parametrize("name", lf.GOLDEN_FILES)
def test_golden_files_equal_pillow(name, golden_dir):
    data = open(os.path.join(golden_dir, name), "rb").read()
    assert mismatches(reference_rgb(data), pillow_rgb(data)) == 0


# ---- Pillow-written files
def source_image(kind, w, h):
    if kind == "noise":
        return np.random.default_rng(w * 131 + h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    photo = pillow_rgb(open(os.path.join(ROOT, "tests", "golden", "Mouse480.jpg"), "rb").read())
    return np.ascontiguousarray(photo[100:100 + h, 150:150 + w])


PILLOW_SIZES = [(5, 5), (17, 9), (53, 45), (64, 48), (200, 120)]


@pytest.mark.parametrize("quality", [30, 75, 95, 100])
@pytest.mark.parametrize("kind", ["noise", "photo"])
def test_pillow_written_files_equal_pillow(kind, quality):
    Image = pil()
    bad = n = 0
    for w, h in PILLOW_SIZES:
        rgb = source_image(kind, w, h)
        for sub in (0, 1, 2, "grey"):   # 4:4:4, 4:2:2, 4:2:0, one component
            buf = io.BytesIO()
            if sub == "grey":
                Image.fromarray(rgb[..., 1], "L").save(buf, "JPEG", quality=quality)
            else:
                Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=quality, subsampling=sub)
            data = buf.getvalue()
            bad += mismatches(reference_rgb(data), pillow_rgb(data))
            if sub == 0:   # the planes themselves: the block stage in isolation
                info, planes = reference_planes(data)
                ycc = pillow_ycc(data)
                for k in range(3):
                    bad += mismatches(planes[k][:h, :w], ycc[..., k])
            n += 1
    assert n == 20 and bad == 0


# ---- writer-made files
@pytest.mark.parametrize("sampling", [420, 422, 444, 400])
@pytest.mark.parametrize("fam", range(len(lf.FAMILIES)))
def test_writer_made_files_equal_pillow(fam, sampling):
    bad = 0
    for w, h in lf.SIZES:
        data, q, c, planes = lf.writer_file(lf.seed_of(w, h, sampling, fam), w, h, sampling, lf.FAMILIES[fam])
        want = pillow_rgb(data)
        bad += mismatches(lj.record_to_rgb(c, q, planes, sampling, w, h), want)
        bad += mismatches(reference_rgb(data), want)   # ... and through the library's host reader
    assert bad == 0


def test_dense_blocks_under_moderate_tables_equal_pillow():
    """the dense family with q <= 64 (with q <= 255 libjpeg-turbo's SIMD wraps its 16-bit intermediates: the definition is
    the formula, and that family is not held against Pillow)"""
    data, q, c, planes = lf.writer_file(31, 64, 48, 400, lf.DENSE_Q64)
    assert mismatches(lj.record_to_rgb(c, q, planes, 400, 64, 48), pillow_rgb(data)) == 0


def test_restart_intervals_do_not_change_the_image():
    case = (64, 48, 420, 0, 3)
    data, q, c, planes = lf.pinned_file(case)
    from video_coding_amd import hvc
    info, coefs = hvc.jpeg_entropy_decode(data, restart_markers=True)
    assert np.array_equal(coefs, c)
    assert mismatches(lj.record_to_rgb(c, q, planes, 420, 64, 48), pillow_rgb(data)) == 0


# ---- the filter's own rules
@pytest.mark.parametrize("cw,ch", [(1, 1), (2, 3), (3, 1), (3, 2), (9, 5), (27, 23)])
def test_fancy_filter_edges_and_small_windows(cw, ch):
    s = np.random.default_rng(cw * 100 + ch).integers(0, 256, size=(ch, cw), dtype=np.uint8)
    h2, hv2 = lj.fancy_h2(s), lj.fancy_hv2(s)
    assert h2.shape == (ch, 2 * cw) and hv2.shape == (2 * ch, 2 * cw)
    if cw <= 2:
        assert np.array_equal(h2, np.repeat(s, 2, axis=1)) and np.array_equal(hv2, np.repeat(np.repeat(s, 2, axis=0), 2, axis=1))
        return
    assert np.array_equal(h2[:, 0], s[:, 0]) and np.array_equal(h2[:, -1], s[:, -1])
    flat = np.full((ch, cw), 77, dtype=np.uint8)   # a flat window stays flat, edges included
    assert (lj.fancy_h2(flat) == 77).all() and (lj.fancy_hv2(flat) == 77).all()
    # clamped neighbours give the edge rules: the kernel's form
    p = np.pad(s.astype(np.int64), 1, mode="edge")
    t0, t1 = 3 * p[1:-1] + p[:-2], 3 * p[1:-1] + p[2:]
    for r, t in ((0, t0), (1, t1)):
        assert np.array_equal(hv2[r::2, 0::2], (3 * t[:, 1:-1] + t[:, :-2] + 8) >> 4)
        assert np.array_equal(hv2[r::2, 1::2], (3 * t[:, 1:-1] + t[:, 2:] + 7) >> 4)
    assert np.array_equal(h2[:, 0::2], (3 * p[1:-1, 1:-1] + p[1:-1, :-2] + 1) >> 2)
    assert np.array_equal(h2[:, 1::2], (3 * p[1:-1, 1:-1] + p[1:-1, 2:] + 2) >> 2)


def test_junk_beyond_the_window_does_not_matter():
    rng = np.random.default_rng(3)
    for sampling, (w, h) in ((420, (17, 9)), (422, (5, 5)), (420, (3, 2))):
        cw, ch = lj.chroma_window(sampling, w, h)
        planes = [rng.integers(0, 256, size=(h + 16, w + 16), dtype=np.uint8) for _ in range(3)]
        got = lj.planes_to_rgb(planes[0], planes[1], planes[2], sampling, w, h)
        for p in planes[1:]:
            p[ch:, :] ^= 0xff
            p[:, cw:] ^= 0xff
        assert np.array_equal(lj.planes_to_rgb(planes[0], planes[1], planes[2], sampling, w, h), got)


# ---- the pins
def test_pins_are_what_pillow_decodes_today():
    pil()
    import make_libjpeg_pins
    with open(os.path.join(ROOT, "tests", "golden", "libjpeg_pins.json")) as f:
        stored = json.load(f)
    assert make_libjpeg_pins.pins()["rgb_sha256"] == stored["rgb_sha256"]


def test_reference_reproduces_the_pins(golden_dir):
    """without Pillow: the definition against the stored hashes"""
    with open(os.path.join(golden_dir, "libjpeg_pins.json")) as f:
        stored = json.load(f)["rgb_sha256"]
    assert len(stored) == len(lf.GOLDEN_FILES) + len(lf.PINNED)
    for name in lf.GOLDEN_FILES:
        assert lf.sha256(reference_rgb(open(os.path.join(golden_dir, name), "rb").read())) == stored[name]
    for case in lf.PINNED:
        data, q, c, planes = lf.pinned_file(case)
        assert lf.sha256(lj.record_to_rgb(c, q, planes, case[2], case[0], case[1])) == stored[lf.pin_name(*case)]


# ---- header, binding, command line
def test_header_names_the_setting():
    header = open(os.path.join(ROOT, "include", "hvc_jpeg.h")).read()
    assert re.search(r"typedef enum \{ HVC_ARITH_MODEL = 0, HVC_ARITH_HARDCAML = 1, HVC_ARITH_LIBJPEG = 3 \} hvc_arith;", header)
    assert "Bit-exact to libjpeg" in header and "The value 2 is NOT an arithmetic" in header
    spec = lj.spec_constants()
    assert re.search(r"SUM \|d\[k\]\| <= %d in int32" % spec["HVC_IS_GUARD_SUM"], header)


def test_binding_maps_libjpeg():
    from video_coding_amd import hvc
    assert hvc.HVC_ARITH["libjpeg"] == 3 and hvc.HVC_ARITH["model"] == 0 and hvc.HVC_ARITH["hardcaml"] == 1
    assert 2 not in hvc.HVC_ARITH.values()


def test_cli_parses_arithmetic_libjpeg():
    import video_coding_amd.__main__ as cli
    a = cli.parser().parse_args("model decode frame in.jpg out.ppm -rgb -arithmetic libjpeg".split())
    assert a.arithmetic == "libjpeg" and a.rgb and a.fn is cli.model_decode_frame
    assert cli.parser().parse_args("model decode frame in.jpg".split()).arithmetic == "model"
    with pytest.raises(SystemExit):
        cli.parser().parse_args("model decode frame in.jpg -arithmetic turbo".split())


def test_cli_refuses_libjpeg_with_scale_before_any_gpu_call(tmp_path, monkeypatch):
    import video_coding_amd.__main__ as cli

    def no_gpu(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(cli.hvc, "Context", no_gpu)
    with pytest.raises(SystemExit):
        cli.main(["model", "decode", "frame", str(tmp_path / "in.jpg"), "-arithmetic", "libjpeg", "-scale", "2"])
