"""hvc_set_mixed_arithmetic / hvc_get_mixed_arithmetic above the kernels, without a GPU: the header, the Python binding, the
OCaml binding and the command line (`model decode frames ... -arithmetic libjpeg`)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hvc_set_mixed_arithmetic", "hvc_get_mixed_arithmetic"]


def test_header_declares_the_two_functions():
    header = open(os.path.join(ROOT, "include", "hvc_jpeg.h")).read()
    assert re.search(r"HVC_API int hvc_set_mixed_arithmetic\(hvc_ctx \*ctx, int arith\);", header)
    assert re.search(r"HVC_API int hvc_get_mixed_arithmetic\(const hvc_ctx \*ctx, int \*arith\);", header)
    assert "their libjpeg forms are not built yet" not in header      # the sentence that called the mixed form a later step
    assert "k_islow_mixed" in header and "k_ycc_to_rgb_fancy_mixed" in header


def test_python_binding_names_them():
    from video_coding_amd import hvc
    for name in NAMES:
        assert name in hvc.SYMBOLS
    assert callable(hvc.Context.set_mixed_arithmetic) and isinstance(hvc.Context.mixed_arithmetic, property)


def test_library_exports_them_and_refuses_null():
    import ctypes
    import video_coding_amd as m
    m.build()
    L = m.lib()
    v = ctypes.c_int(-5)
    assert L.hvc_set_mixed_arithmetic(None, 3) == -1 and L.hvc_set_mixed_arithmetic(None, 0) == -1
    assert L.hvc_get_mixed_arithmetic(None, ctypes.byref(v)) == -1 and v.value == -5


def test_ocaml_binding_names_them():
    ml = open(os.path.join(ROOT, "integration", "ocaml", "hvc.ml")).read()
    for name in NAMES:
        assert re.search(r'foreign\s+"%s"' % name, ml), name


def test_cli_parses_decode_frames_arithmetic_libjpeg():
    import video_coding_amd.__main__ as cli
    a = cli.parser().parse_args("model decode frames out a.jpg b.jpg -rgb -arithmetic libjpeg".split())
    assert a.arithmetic == "libjpeg" and a.rgb and a.bits == ["a.jpg", "b.jpg"] and a.out_dir == "out" and a.fn is cli.model_decode_frames
    assert cli.parser().parse_args("model decode frames out a.jpg".split()).arithmetic == "model"
    a = cli.parser().parse_args("model decode frames out a.jpg -rgb -resize 24x16 -filter bicubic -reader gpu -arithmetic libjpeg".split())
    assert a.arithmetic == "libjpeg" and a.resize == (24, 16) and a.filter == "bicubic" and a.reader == "gpu"
    for bad in ("hardcaml", "turbo"):
        with pytest.raises(SystemExit):
            cli.parser().parse_args(("model decode frames out a.jpg -arithmetic " + bad).split())


@pytest.mark.parametrize("extra", [[], ["-rgb"], ["-rgb", "-resize", "24x16"]])
def test_cli_refuses_libjpeg_with_scale_before_any_context(tmp_path, monkeypatch, extra):
    import video_coding_amd.__main__ as cli

    def no_gpu(*a, **k):
        raise AssertionError("a context was created")
    monkeypatch.setattr(cli.hvc, "Context", no_gpu)
    with pytest.raises(SystemExit) as e:
        cli.main(["model", "decode", "frames", str(tmp_path / "out"), str(tmp_path / "a.jpg"), str(tmp_path / "b.jpg"), "-arithmetic", "libjpeg",
                  "-scale", "2"] + extra)
    assert "-scale" in str(e.value.code)
    assert not (tmp_path / "out").exists()
