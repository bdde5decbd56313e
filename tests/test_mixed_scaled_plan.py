"""The host plan of a mixed batch at 1/2, 1/4, 1/8 size, without a GPU: the descriptor builder for k_decode_mixed_scaled
(csrc/hvc_mixed_plan.cpp with n = 4, 2, 1) and the colour plan over scaled planes (csrc/hvc_mixed_rgb_plan.cpp) through the
stand-alone program tests/host_harness/mixed_scaled_plan_harness.cpp -- a CPU-only g++ build under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/host_harness/Makefile.mixed_scaled) -- and hvc_jpeg_mixed_scaled_layout /
hvc_jpeg_mixed_scaled_rgb_layout through the library.  Nothing loaded into Python runs under a sanitizer."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import golden_bytes
from test_host_entropy import UNUSUAL_SAMPLINGS, unusual_sampling_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
SCALES = (2, 4, 8)


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixed_scaled") / "mixed_scaled_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.mixed_scaled", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def files():
    """golden files and unusual samplings (odd sizes among them), with a truncated file and a progressive SOF in the middle"""
    mini = golden_bytes("mini.jpg")
    out = [mini, golden_bytes("Mouse480.jpg")]
    out += [unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 70, 38, 7 * si)[0] for si in (0, 3, 9)]
    out.append(mini[:100])                                    # no SOS: HVC_E_BAD_JPEG
    out.append(mini.replace(b"\xff\xc0", b"\xff\xc2", 1))     # SOF2: HVC_E_UNSUPPORTED_MARKER
    out += [unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 97, 51, 7 * si + 1)[0] for si in (1, 8, 11)]
    return out


def run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_squares_flags_and_the_full_size_plan(harness):
    """planes of 1, 63, 64, 65, 256, 257 blocks, bw in 1, 5, 6, 9, an empty plane; N = 4, 2, 1; tight, on 4 bytes, shifted by a
    byte; two base addresses: every square inside its record, disjoint, covering; the dword flag; units, map, tables as at
    full size"""
    assert run(harness, "shapes").split() == ["ok", "18"]


def test_seeded_random_sets_in_the_sanitizer_build(harness):
    assert run(harness, "random", 20261018, 300).split() == ["ok", "300"]


def test_the_colour_plan_refuses_a_window_beyond_the_scaled_planes(harness):
    assert run(harness, "window").split() == ["ok"]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("align", [8, 256, 0])
def test_layout_offsets(hvc, files, scale, align):
    lay = hvc.jpeg_mixed_scaled_layout(files, scale, align)
    a = align or 256
    end = 0
    assert [lay.status[f] for f in (5, 6)] == [-8, -9]
    for f, data in enumerate(files):
        if f in (5, 6):
            continue
        assert lay.status[f] == 0, f
        full = hvc.jpeg_read_header(data)
        assert bytes(lay.infos[f]) == bytes(full)                                  # the batch call's input: the FULL-size info
        assert bytes(lay.scaled[f]) == bytes(hvc.jpeg_scaled_info(full, scale))    # byte for byte
        off = lay.pixel_offsets[f]
        assert off % a == 0 and off >= end and off - end < a   # aligned, behind the last record, no more than the rounding apart
        end = off + lay.scaled[f].pixel_bytes
    assert lay.total_bytes == end                              # exact: the failed files took no room


def test_scale_1_is_the_full_size_layout(hvc, files):
    for align in (8, 64):
        a, b = hvc.jpeg_mixed_scaled_layout(files, 1, align), hvc.jpeg_mixed_layout(files, align)
        assert a.total_bytes == b.total_bytes and list(a.status) == list(b.status) and list(a.pixel_offsets) == list(b.pixel_offsets)
        for f in range(len(files)):
            if b.status[f] == 0:
                assert bytes(a.infos[f]) == bytes(b.infos[f]) == bytes(a.scaled[f])
    with pytest.raises(hvc.HvcError) as e:                     # ... with its rules: align below 8
        hvc.jpeg_mixed_scaled_layout(files, 1, 4)
    assert e.value.code == -1


def test_layout_arguments(hvc, files):
    for bad in (0, 3, 16, -2):
        with pytest.raises(hvc.HvcError) as e:
            hvc.jpeg_mixed_scaled_layout(files, bad)
        assert e.value.code == -1
        with pytest.raises(hvc.HvcError) as e:
            hvc.jpeg_mixed_scaled_rgb_layout(files, bad)
        assert e.value.code == -1
    for bad in (12, 4, 1, 24):
        with pytest.raises(hvc.HvcError) as e:
            hvc.jpeg_mixed_scaled_layout(files, 2, bad)
        assert e.value.code == -1
    only_bad = hvc.jpeg_mixed_scaled_layout(files[5:7], 4, 8)
    assert list(only_bad.status) == [-8, -9] and only_bad.total_bytes == 0
    assert hvc.jpeg_mixed_scaled_layout([], 8).total_bytes == 0
    L = hvc.lib()
    assert L.hvc_jpeg_mixed_scaled_layout(None, None, 0, 2, 0, None, None, None, None, None) == -1
    assert L.hvc_jpeg_mixed_scaled_rgb_layout(None, None, 0, 2, 0, 0, 0, None, None, None, None, None, None) == -1


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_rgb_layout(hvc, files, layout):
    planar = layout == "planar"
    for scale, row_align in ((2, 1), (4, 8), (8, 0)):
        lay = hvc.jpeg_mixed_scaled_rgb_layout(files, scale, layout, 64, row_align)
        full = hvc.jpeg_mixed_rgb_layout(files, layout, 64, row_align)
        assert list(lay.status) == list(full.status)           # the same files have an image (header and sampling)
        end = 0
        for f in range(len(files)):
            if lay.status[f]:
                assert lay.rgb_row_strides[f] == 0
                continue
            s = hvc.jpeg_scaled_info(hvc.jpeg_read_header(files[f]), scale)
            assert bytes(lay.scaled[f]) == bytes(s)
            ra = row_align or 1
            row = -(-(s.width if planar else 3 * s.width) // ra) * ra
            assert lay.rgb_row_strides[f] == row
            off = lay.rgb_offsets[f]
            assert off % 64 == 0 and off >= end and off - end < 64
            end = off + row * s.height * (3 if planar else 1)
        assert lay.total_bytes == end
    one = hvc.jpeg_mixed_scaled_rgb_layout(files, 1, layout, 64, 8)
    ref = hvc.jpeg_mixed_rgb_layout(files, layout, 64, 8)
    assert one.total_bytes == ref.total_bytes and list(one.rgb_offsets) == list(ref.rgb_offsets)
    assert list(one.rgb_row_strides) == list(ref.rgb_row_strides)


def test_layout_in_the_sanitizer_build(hvc, harness, files, tmp_path):
    paths = []
    for k, f in enumerate(files):
        p = tmp_path / ("f%d.jpg" % k)
        p.write_bytes(f)
        paths.append(str(p))
    for scale, align in ((2, 8), (8, 256), (1, 8)):
        lines = run(harness, "layout", scale, align, *paths).splitlines()
        lay = hvc.jpeg_mixed_scaled_layout(files, scale, align)
        assert lines[0] == "status 0 total %d" % lay.total_bytes
        for f in range(len(files)):
            assert lines[1 + f] == "file %d %d %d %d" % (f, lay.status[f], lay.pixel_offsets[f],
                                                        0 if lay.status[f] else lay.scaled[f].pixel_bytes)
    assert run(harness, "layout", 3, 8, *paths).split()[:2] == ["status", "-1"]
    assert run(harness, "layout", 2, 12, *paths).split()[:2] == ["status", "-1"]
