"""The six layout classes of the binding against the C calls they wrap, made by hand through hvc.lib(): every member equal,
for a file set with a file that fails and for a frame list with a frame that is refused, and all six on an empty list.
The layout calls are host code: no GPU, no context."""
import ctypes as C
import os

import pytest

from video_coding_amd import hvc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HVC_E_TRUNCATED = -8   # what the first 100 bytes of mini.jpg answer


def _read(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module", autouse=True)
def built_library():
    hvc.build()


@pytest.fixture(scope="module")
def files():
    mini = _read("mini.jpg")
    return [mini, mini[:100], _read("Mouse480.jpg")]


FRAMES = [(16, 16, 420, 75), (17, 9, 444, 50), (16, 16, 411, 75)]   # the last one: no such sampling, refused


def _raw(arr):
    return bytes(memoryview(arr).cast("B")) if len(arr) else b""


def _by_hand(name, files, middle, n_infos, n_arrays):
    """name(ptrs, sizes, n, *middle, n_infos x infos, status, n_arrays x size_t array, &total) -> (infos..., status, arrays..., total)"""
    n = len(files)
    ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(j), C.c_void_p) for j in files])
    sizes = (C.c_size_t * n)(*[len(j) for j in files])
    infos = [(hvc.JpegInfo * n)() for _ in range(n_infos)]
    status = (C.c_int * n)()
    arrays = [(C.c_size_t * n)() for _ in range(n_arrays)]
    total = C.c_size_t(0)
    assert getattr(hvc.lib(), name)(ptrs, sizes, n, *middle, *infos, status, *arrays, C.byref(total)) == 0
    return infos, status, arrays, total.value


def _check_file_set(lay, files, infos, status, arrays, total, names, scaled):
    assert len(lay) == len(files)
    assert lay.jpegs == list(files)
    assert list(lay.sizes) == [len(j) for j in files]
    assert len(lay.ptrs) == len(files)
    for p, j in zip(lay.ptrs, files):
        assert C.string_at(p, len(j)) == j
    assert list(lay.status) == list(status)
    assert _raw(lay.infos) == _raw(infos[0])
    assert hasattr(lay, "scaled") == scaled
    if scaled:
        assert _raw(lay.scaled) == _raw(infos[1])
    for name, want in zip(names, arrays):
        assert list(getattr(lay, name)) == list(want), name
    assert lay.total_bytes == total


def _expect_statuses(status):
    assert list(status) == [0, HVC_E_TRUNCATED, 0]


@pytest.mark.parametrize("align", [0, 4096])
def test_mixed_layout(files, align):
    infos, status, arrays, total = _by_hand("hvc_jpeg_mixed_layout", files, (align,), 1, 1)
    _expect_statuses(status)
    for lay in (hvc.MixedLayout(files, align), hvc.jpeg_mixed_layout(files, align)):
        _check_file_set(lay, files, infos, status, arrays, total, ["pixel_offsets"], False)
    assert total > 0 and all(o % (align or 256) == 0 for o in arrays[0])


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("row_align", [0, 64])
@pytest.mark.parametrize("align", [0, 4096])
def test_mixed_rgb_layout(files, align, row_align, layout):
    code = hvc.HVC_RGB[layout]
    infos, status, arrays, total = _by_hand("hvc_jpeg_mixed_rgb_layout", files, (code, align, row_align), 1, 2)
    _expect_statuses(status)
    for lay in (hvc.MixedRgbLayout(files, layout, align, row_align), hvc.jpeg_mixed_rgb_layout(files, layout, align, row_align)):
        _check_file_set(lay, files, infos, status, arrays, total, ["rgb_offsets", "rgb_row_strides"], False)
        assert lay.layout == code


@pytest.mark.parametrize("scale_denom", [2, 8])
@pytest.mark.parametrize("align", [0, 4096])
def test_mixed_scaled_layout(files, align, scale_denom):
    infos, status, arrays, total = _by_hand("hvc_jpeg_mixed_scaled_layout", files, (scale_denom, align), 2, 1)
    _expect_statuses(status)
    for lay in (hvc.MixedScaledLayout(files, scale_denom, align), hvc.jpeg_mixed_scaled_layout(files, scale_denom, align)):
        _check_file_set(lay, files, infos, status, arrays, total, ["pixel_offsets"], True)
        assert lay.scale_denom == scale_denom
    assert infos[1][0].width == -(-infos[0][0].width // scale_denom)


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("scale_denom", [2, 8])
@pytest.mark.parametrize("align,row_align", [(0, 0), (4096, 0), (0, 64), (4096, 64)])
def test_mixed_scaled_rgb_layout(files, align, row_align, scale_denom, layout):
    code = hvc.HVC_RGB[layout]
    infos, status, arrays, total = _by_hand("hvc_jpeg_mixed_scaled_rgb_layout", files, (scale_denom, code, align, row_align), 2, 2)
    _expect_statuses(status)
    for lay in (hvc.MixedScaledRgbLayout(files, scale_denom, layout, align, row_align),
                hvc.jpeg_mixed_scaled_rgb_layout(files, scale_denom, layout, align, row_align)):
        _check_file_set(lay, files, infos, status, arrays, total, ["rgb_offsets", "rgb_row_strides"], True)
        assert lay.scale_denom == scale_denom and lay.layout == code


def _columns(frames, m):
    return [(C.c_int * m)(*[f[k] for f in frames]) for k in range(4)]


def _check_encoder(lay, frames, infos, status, arrays, names):
    n = len(frames)
    assert len(lay) == lay.n == n
    assert _raw(lay.infos) == _raw(infos)
    assert list(lay.status) == list(status)
    for name, want in zip(names, arrays):
        assert list(getattr(lay, name)) == list(want), name
    for f, (w, h, _, _) in enumerate(frames):
        if status[f] == 0:
            assert (lay.infos[f].width, lay.infos[f].height) == (w, h)


@pytest.mark.parametrize("align", [0, 4096])
def test_encoder_mixed_layout(align):
    n = m = len(FRAMES)
    infos, status = (hvc.JpegInfo * m)(), (C.c_int * m)()
    po, co, pt, ct = (C.c_size_t * m)(), (C.c_size_t * m)(), C.c_size_t(), C.c_size_t()
    assert hvc.lib().hvc_jpeg_encoder_mixed_layout(*_columns(FRAMES, m), n, align, infos, status, po, co, C.byref(pt), C.byref(ct)) == 0
    assert status[0] == 0 and status[1] == 0 and status[2] != 0
    for lay in (hvc.EncoderMixedLayout(FRAMES, align), hvc.jpeg_encoder_mixed_layout(FRAMES, align)):
        _check_encoder(lay, FRAMES, infos, status, [po, co], ["pixel_offsets", "coef_offsets"])
        assert (lay.pixel_total, lay.coef_total) == (pt.value, ct.value)
        assert not hasattr(lay, "total_bytes")
    assert pt.value > 0 and ct.value > 0


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("align,row_align", [(0, 0), (4096, 0), (0, 64), (4096, 64)])
def test_encoder_mixed_rgb_layout(align, row_align, layout):
    n = m = len(FRAMES)
    code = hvc.HVC_RGB[layout]
    infos, status = (hvc.JpegInfo * m)(), (C.c_int * m)()
    ro, rs, po, co = [(C.c_size_t * m)() for _ in range(4)]
    rt, pt, ct = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert hvc.lib().hvc_jpeg_encoder_mixed_rgb_layout(*_columns(FRAMES, m), n, code, align, row_align, infos, status, ro, rs,
                                                       C.byref(rt), po, co, C.byref(pt), C.byref(ct)) == 0
    assert status[0] == 0 and status[2] != 0   # (17 x 9 4:4:4 is a frame the RGB form takes too: 4:4:4 has no even-size rule)
    assert status[1] == 0
    for lay in (hvc.EncoderMixedRgbLayout(FRAMES, layout, align, row_align),
                hvc.jpeg_encoder_mixed_rgb_layout(FRAMES, layout, align, row_align)):
        assert isinstance(lay, hvc.EncoderMixedLayout)
        _check_encoder(lay, FRAMES, infos, status, [ro, rs, po, co], ["rgb_offsets", "rgb_row_strides", "pixel_offsets", "coef_offsets"])
        assert lay.layout == code
        assert lay.total_bytes == lay.rgb_total == rt.value
        assert (lay.pixel_total, lay.coef_total) == (pt.value, ct.value)


def test_all_six_on_an_empty_list():
    for lay in (hvc.MixedLayout([]), hvc.MixedRgbLayout([]), hvc.MixedScaledLayout([], 2), hvc.MixedScaledRgbLayout([], 2)):
        assert len(lay) == 0 and lay.jpegs == [] and lay.total_bytes == 0
        assert len(lay.ptrs) == len(lay.sizes) == len(lay.infos) == len(lay.status) == 0
    enc, enc_rgb = hvc.EncoderMixedLayout([]), hvc.EncoderMixedRgbLayout([])
    for lay in (enc, enc_rgb):
        assert len(lay) == 0 and (lay.pixel_total, lay.coef_total) == (0, 0)
    assert not hasattr(enc, "total_bytes")
    assert enc_rgb.total_bytes == enc_rgb.rgb_total == 0
