"""The host plan of the colour pass over a mixed batch (csrc/hvc_mixed_rgb_plan.cpp), without a GPU:
hvc_jpeg_mixed_rgb_layout through the library, the descriptor builder through the stand-alone program
tests/host_harness/mixed_rgb_plan_harness.cpp -- which keeps the builder out of the public header and runs it, and the layout
call, under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only g++ build: tests/host_harness/Makefile.mixed_rgb).
Nothing loaded into Python runs under a sanitizer."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import golden_bytes
from test_host_entropy import unusual_sampling_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}

FACTORS = {420: [(2, 2), (1, 1), (1, 1)], 422: [(2, 1), (1, 1), (1, 1)], 444: [(1, 1)] * 3, 400: [(1, 1)]}
CONVERTIBLE = [FACTORS[420], FACTORS[422], FACTORS[444], FACTORS[400], [(2, 2)]]          # read as 420, 422, 444, grey, grey
UNCONVERTIBLE = [[(4, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(2, 1), (1, 1)]]    # 4:1:1, 4:4:0, two components


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixed_rgb") / "mixed_rgb_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.mixed_rgb", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def files():
    """golden files, convertible and unconvertible samplings, with a truncated file and a progressive SOF in the middle"""
    mini = golden_bytes("mini.jpg")
    out = [mini, golden_bytes("Mouse480.jpg")]
    out += [unusual_sampling_file(s, 40, 24, 7 * k)[0] for k, s in enumerate(CONVERTIBLE)]
    out.append(unusual_sampling_file(UNCONVERTIBLE[0], 40, 24, 50)[0])
    out.append(mini[:100])                                    # no SOS: HVC_E_BAD_JPEG
    out.append(mini.replace(b"\xff\xc0", b"\xff\xc2", 1))     # SOF2: HVC_E_UNSUPPORTED_MARKER
    out += [unusual_sampling_file(s, 97, 51, 60 + k)[0] for k, s in enumerate(UNCONVERTIBLE[1:] + CONVERTIBLE[:2])]
    return out


WANT_STATUS = [0, 0, 0, 0, 0, 0, 0, -1, -8, -9, -1, -1, 0, 0]


@pytest.mark.parametrize("layout", ["interleaved", "planar"])
@pytest.mark.parametrize("row_align", [0, 8, 64])
@pytest.mark.parametrize("align", [1, 8, 256, 0])
def test_layout_offsets(hvc, files, align, row_align, layout):
    lay = hvc.jpeg_mixed_rgb_layout(files, layout, align, row_align)
    a, ra = align or 256, row_align or 1
    assert list(lay.status) == WANT_STATUS
    end = 0
    for f, data in enumerate(files):
        if lay.status[f]:
            continue
        info = hvc.jpeg_read_header(data)
        assert bytes(lay.infos[f]) == bytes(info)
        tight = info.width * (1 if layout == "planar" else 3)
        stride = lay.rgb_row_strides[f]
        assert stride % ra == 0 and tight <= stride < tight + ra        # the tight row rounded up to row_align
        off = lay.rgb_offsets[f]
        assert off % a == 0 and off >= end and off - end < a            # aligned, behind the last record, no more than the rounding apart
        end = off + stride * info.height * (3 if layout == "planar" else 1)
    assert lay.total_bytes == end                                       # exact: failed and unconvertible files took no room


def test_layout_arguments(hvc, files):
    for align, row_align in ((12, 0), (0, 3), (24, 8), (8, 48)):
        with pytest.raises(hvc.HvcError) as e:
            hvc.jpeg_mixed_rgb_layout(files, "interleaved", align, row_align)
        assert e.value.code == -1
    with pytest.raises(hvc.HvcError) as e:
        hvc.jpeg_mixed_rgb_layout(files, 2)
    assert e.value.code == -1
    one = hvc.jpeg_mixed_rgb_layout(files[:1])
    assert len(one) == 1 and one.status[0] == 0 and one.rgb_offsets[0] == 0 and one.rgb_row_strides[0] == 3 * 64
    assert one.total_bytes == 3 * 64 * 64
    only_bad = hvc.jpeg_mixed_rgb_layout(files[7:10], "planar", 8, 8)
    assert list(only_bad.status) == [-1, -8, -9] and only_bad.total_bytes == 0
    assert hvc.jpeg_mixed_rgb_layout([]).total_bytes == 0


def test_layout_in_the_sanitizer_build(hvc, harness, files, tmp_path):
    paths = []
    for k, f in enumerate(files):
        p = tmp_path / ("f%d.jpg" % k)
        p.write_bytes(f)
        paths.append(str(p))
    for layout, align, row_align in ((0, 1, 0), (1, 256, 8), (0, 0, 64)):
        r = subprocess.run([harness, "layout", str(layout), str(align), str(row_align)] + paths, capture_output=True, text=True, env=ENV)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        lines = r.stdout.splitlines()
        lay = hvc.jpeg_mixed_rgb_layout(files, layout, align, row_align)
        assert lines[0] == "status 0 total %d" % lay.total_bytes
        for f in range(len(files)):
            assert lines[1 + f] == "file %d %d %d %d" % (f, lay.status[f], lay.rgb_offsets[f], lay.rgb_row_strides[f])
    r = subprocess.run([harness, "layout", "0", "12", "0"] + paths, capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and r.stdout.split()[:2] == ["status", "-1"]


# ---------------------------------------------------------------------------
# the descriptor builder

def make_image(hvc, w, h, sampling, pad_w=0, decoded=True):
    """a JpegInfo of a w x h image of that sampling: planes back to back, every plane as the block stage decodes it
    (decoded: whole blocks, stride = blocks_w * 8) or raw (the window itself, stride = its width + pad_w, no blocks named)"""
    info = hvc.JpegInfo()
    info.width, info.height = w, h
    fac = FACTORS[sampling]
    info.n_comp, info.n_qtabs = len(fac), 1
    cw, ch = hvc.rgb_chroma_window(sampling, w, h)
    po = 0
    for i, (hs, vs) in enumerate(fac):
        info.comp[i].hscale, info.comp[i].vscale = hs, vs
        pw, ph = (w, h) if i == 0 else (cw, ch)
        L = info.layout[i]
        if decoded:
            L.blocks_w, L.blocks_h = max(-(-pw // 8), 1), max(-(-ph // 8), 1)
            L.stride, rows = L.blocks_w * 8, L.blocks_h * 8
        else:
            L.stride, rows = pw + pad_w, ph
        L.coef_offset, L.plane_offset = po, po
        po += L.stride * rows
    info.coef_count, info.pixel_bytes = po, po
    return info


FIELDS = ("frame", "y_base", "cb_base", "cr_base", "rgb_base", "y_stride", "cb_stride", "cr_stride", "row_stride", "plane_stride",
          "w", "h", "cw", "ch", "sampling", "vec_y", "vec_c", "vec_rgb", "groups", "magic", "lanes", "unit0")


def run_builder(harness, tmp_path, infos, yuv_offsets, rgb_offsets, strides=None, layout=0, frames=None, yuv_addr=0, rgb_addr=0,
                decoded=False):
    n = len(infos)
    raw = struct.pack("<7q", n, -1 if frames is None else len(frames), layout, yuv_addr, rgb_addr, int(decoded), int(strides is not None))
    raw += b"".join(bytes(i) for i in infos)
    raw += struct.pack("<%dQ" % n, *yuv_offsets) + struct.pack("<%dQ" % n, *rgb_offsets) + struct.pack("<%dQ" % n, *(strides or [0] * n))
    if frames is not None:
        raw += struct.pack("<%di" % len(frames), *frames)
    p = tmp_path / "set.bin"
    p.write_bytes(raw)
    r = subprocess.run([harness, "dump", str(p)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(images=[], map=[])
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] in ("status", "lanes"):
            out[w[0]] = int(w[1])
        elif w[0] == "check":
            out["check"] = " ".join(w[1:])
        elif w[0] == "image":
            out["images"].append(dict(zip(FIELDS, map(int, w[2:]))))
        elif w[0] == "map":
            out["map"] = list(map(int, w[1:]))
    return out


def place(infos, layout=0, align=256):
    yuv, rgb, yo, ro = [], [], 0, 0
    for i in infos:
        yuv.append(yo)
        rgb.append(ro)
        yo += -(-i.pixel_bytes // 256) * 256
        ro += -(-(3 * i.width * i.height) // align) * align
    return yuv, rgb


def test_every_lane_has_exactly_one_unit_and_lane(hvc, harness, tmp_path):
    """images of 1, 63, 64, 65, 256 and 257 lanes, one lane per row with 257 rows, an image without a pixel in the middle"""
    infos = [
        make_image(hvc, 8, 1, 444),        # 1
        make_image(hvc, 72, 14, 420),      # 9 x 7 = 63
        make_image(hvc, 64, 16, 420),      # 8 x 8 = 64
        make_image(hvc, 40, 0, 422),       # h = 0: no descriptor
        make_image(hvc, 40, 26, 420),      # 5 x 13 = 65
        make_image(hvc, 128, 16, 422),     # 16 x 16 = 256
        make_image(hvc, 2050, 1, 444),     # 257 x 1
        make_image(hvc, 7, 257, 400),      # one lane per row, 257 rows
    ]
    yuv, rgb = place(infos)
    plan = run_builder(harness, tmp_path, infos, yuv, rgb, decoded=True)
    assert plan["status"] == 0 and plan["check"] == "ok"
    im = plan["images"]
    assert [k["frame"] for k in im] == [0, 1, 2, 4, 5, 6, 7]
    assert [k["lanes"] for k in im] == [1, 63, 64, 65, 256, 257, 257]
    assert [k["groups"] for k in im] == [1, 9, 8, 5, 16, 257, 1]
    assert [k["sampling"] for k in im] == [444, 420, 420, 420, 422, 444, 400]
    assert [(k["cw"], k["ch"]) for k in im] == [(8, 1), (36, 7), (32, 8), (20, 13), (64, 16), (2050, 1), (0, 0)]
    assert plan["lanes"] == sum(k["lanes"] for k in im)
    want_map = []
    for i, k in enumerate(im):
        assert k["unit0"] == len(want_map)
        want_map += [i] * (-(-k["lanes"] // 64))
    assert plan["map"] == want_map and len(want_map) == 1 + 1 + 1 + 2 + 4 + 5 + 5
    # every lane in exactly one (unit, lane), by the kernel's own arithmetic
    for i, k in enumerate(im):
        lrows = k["lanes"] // k["groups"]
        seen = np.zeros((lrows, k["groups"]), dtype=int)
        for u in [u for u, x in enumerate(plan["map"]) if x == i]:
            for lane in range(64):
                t = (u - k["unit0"]) * 64 + lane
                if t < k["lanes"]:
                    lr = t if k["groups"] == 1 else (t * k["magic"]) >> 32
                    seen[lr, t - lr * k["groups"]] += 1
        assert (seen == 1).all(), i
    # bases: the frame's offset plus the plane's
    assert im[3]["y_base"] == yuv[4] and im[3]["cb_base"] == yuv[4] + infos[4].layout[1].plane_offset
    assert im[3]["rgb_base"] == rgb[4] and im[3]["row_stride"] == 3 * 40


def test_flags_follow_the_actual_bases_and_strides(hvc, harness, tmp_path):
    infos = [make_image(hvc, 64, 16, 420), make_image(hvc, 64, 16, 420), make_image(hvc, 64, 16, 444),
             make_image(hvc, 18, 6, 422, pad_w=1, decoded=False), make_image(hvc, 60, 4, 420)]
    yuv = [0, 4096, 8192, 16384, 20480]
    rgb = [0, 3077, 8192, 16384, 20480]              # image 1: an offset that is odd mod 8
    plan = run_builder(harness, tmp_path, infos, yuv, rgb)
    assert plan["status"] == 0 and plan["check"] == "ok"
    flags = [(k["vec_y"], k["vec_c"], k["vec_rgb"]) for k in plan["images"]]
    assert flags[0] == (1, 1, 1)
    assert flags[1] == (1, 1, 0)                     # the record off 8 bytes
    assert flags[2] == (1, 1, 1)
    assert flags[3] == (0, 0, 0)                     # luma stride 19, chroma stride 10 (off 4), rows of 54 bytes
    assert flags[4] == (1, 1, 0)                     # tight rows of 180 bytes: 8-byte pieces only when width % 8 == 0
    # a row stride on 8 bytes brings the 8-byte stores back; planar planes also need row_stride * h on 8
    plan = run_builder(harness, tmp_path, infos, yuv, rgb, strides=[0, 0, 0, 56, 184])
    assert [k["vec_rgb"] for k in plan["images"]] == [1, 0, 1, 1, 1]
    plan = run_builder(harness, tmp_path, infos, yuv, rgb, strides=[0, 0, 0, 24, 60], layout=1)
    assert [k["vec_rgb"] for k in plan["images"]] == [1, 0, 1, 1, 0] and plan["images"][3]["plane_stride"] == 24 * 6
    # the addresses the offsets count from are part of it
    plan = run_builder(harness, tmp_path, infos, yuv, rgb, yuv_addr=0x7000004, rgb_addr=0x9000003)
    flags = [(k["vec_y"], k["vec_c"], k["vec_rgb"]) for k in plan["images"]]
    assert flags[0] == (0, 1, 0) and flags[1] == (0, 1, 1) and flags[2] == (0, 0, 0)
    # 4:4:4 chroma moves in 8-byte pieces: a plane off 8 but on 4 is not enough
    odd = make_image(hvc, 64, 16, 444)
    odd.layout[1].plane_offset += 4
    plan = run_builder(harness, tmp_path, [odd], [0], [0])
    assert (plan["images"][0]["vec_y"], plan["images"][0]["vec_c"]) == (1, 0)


def test_a_list_of_frames_leaves_the_others_out(hvc, harness, tmp_path):
    infos = [make_image(hvc, 16, 16, 420), make_image(hvc, 600, 3, 444), make_image(hvc, 24, 24, 400)]
    yuv, rgb = place(infos)
    plan = run_builder(harness, tmp_path, infos, yuv, rgb, frames=[2, 0])
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert [k["frame"] for k in plan["images"]] == [2, 0] and [k["lanes"] for k in plan["images"]] == [72, 16]
    assert plan["map"] == [0, 0, 1] and plan["images"][0]["y_base"] == yuv[2] and plan["images"][1]["rgb_base"] == 0
    none = run_builder(harness, tmp_path, infos, yuv, rgb, frames=[])
    assert none["status"] == 0 and none["images"] == [] and none["map"] == [] and none["lanes"] == 0


def test_refusals(hvc, harness, tmp_path):
    ok = make_image(hvc, 40, 24, 420)
    assert run_builder(harness, tmp_path, [ok], [0], [0], decoded=True)["status"] == 0
    assert run_builder(harness, tmp_path, [ok], [0], [0], layout=2)["status"] == -1           # a layout that is neither
    short = make_image(hvc, 40, 24, 420)
    short.layout[0].stride = 39
    assert run_builder(harness, tmp_path, [short], [0], [0])["status"] == -1                  # a stride below its row
    short = make_image(hvc, 40, 24, 420)
    short.layout[2].stride = 19
    assert run_builder(harness, tmp_path, [short], [0], [0])["status"] == -1
    assert run_builder(harness, tmp_path, [ok], [0], [0], strides=[119])["status"] == -1      # an RGB row stride below 3 w
    assert run_builder(harness, tmp_path, [ok], [0], [0], strides=[40], layout=1)["status"] == 0
    out = make_image(hvc, 40, 24, 420)
    out.layout[1].blocks_h = 1                                                                # 12 chroma rows in a plane of 8
    assert run_builder(harness, tmp_path, [out], [0], [0])["status"] == -1
    out = make_image(hvc, 41, 24, 422)
    out.layout[0].blocks_w = 5                                                                # 41 columns in 40
    assert run_builder(harness, tmp_path, [out], [0], [0])["status"] == -1
    raw = make_image(hvc, 40, 24, 420, decoded=False)
    assert run_builder(harness, tmp_path, [raw], [0], [0])["status"] == 0                     # raw planes name no blocks ...
    assert run_builder(harness, tmp_path, [raw], [0], [0], decoded=True)["status"] == -1      # ... which decoded planes must
    for fac in ([(4, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(2, 1), (1, 1)], [(2, 2), (1, 1), (1, 1), (2, 2)]):
        bad = make_image(hvc, 40, 24, 444)
        bad.n_comp = len(fac)
        for i, (hs, vs) in enumerate(fac):
            bad.comp[i].hscale, bad.comp[i].vscale = hs, vs
        assert run_builder(harness, tmp_path, [ok, bad], [0, 4096], [0, 4096])["status"] == -1   # a sampling that is none of the four
        assert run_builder(harness, tmp_path, [ok, bad], [0, 4096], [0, 4096], frames=[0])["status"] == 0
    neg = make_image(hvc, 40, 24, 420)
    neg.width = -1
    assert run_builder(harness, tmp_path, [neg], [0], [0])["status"] == -1
    # HVC_MIXED_MAX_UNITS = 2^26 units: an image of 2 x 2^24 lanes has 2^19 of them, 128 such images are the most
    tall = make_image(hvc, 16, 1 << 24, 400, decoded=False)
    assert run_builder(harness, tmp_path, [tall], [0], [0], frames=[0] * 129)["status"] == -7
    wide = make_image(hvc, 16384, 1024, 400, decoded=False)                                   # lanes * groups = 2^32
    assert run_builder(harness, tmp_path, [wide], [0], [0])["status"] == -7
    huge = make_image(hvc, (1 << 24) + 1, 1, 400, decoded=False)
    assert run_builder(harness, tmp_path, [huge], [0], [0])["status"] == -7


def test_seeded_random_sets_in_the_sanitizer_build(harness):
    r = subprocess.run([harness, "random", "20261018", "400"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.split()[:2] == ["ok", "400"]
