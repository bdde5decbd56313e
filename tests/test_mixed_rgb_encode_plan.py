"""The host plan of the colour pass in front of a mixed ENCODE batch (mixed_rgb_encode_plan_build, csrc/hvc_mixed_rgb_plan.cpp),
without a GPU: the descriptor builder through the stand-alone program tests/host_harness/mixed_rgb_encode_plan_harness.cpp, which
keeps the builder out of the public header and runs it under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only g++
build: tests/host_harness/Makefile.mixed_rgb_encode).  Nothing loaded into Python runs under a sanitizer."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}

FACTORS = {420: [(2, 2), (1, 1), (1, 1)], 422: [(2, 1), (1, 1), (1, 1)], 444: [(1, 1)] * 3}

# (sampling, w, h, lanes): every boundary of the decomposition -- one lane; exactly one unit, one lane short of it, one over it;
# groups == 1 (magic 0); a partial last column group; several units with groups = 17.  tests/test_gpu_mixed_encode_rgb.py runs
# the same set on the GPU.
GEOMETRIES = [(444, 1, 1, 1), (422, 2, 1, 1), (420, 2, 2, 1), (420, 16, 64, 64), (420, 24, 42, 63), (444, 8, 65, 65), (422, 40, 13, 65),
              (444, 8, 3, 3), (420, 6, 4, 2), (422, 10, 3, 6), (420, 18, 10, 15), (420, 136, 66, 561)]


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixed_rgb_encode") / "mixed_rgb_encode_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.mixed_rgb_encode", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def raw_image(hvc, w, h, sampling, pad_w=0):
    """a JpegInfo of a w x h frame whose planes are the samples themselves: stride = the plane's width + pad_w, no blocks named"""
    info = hvc.JpegInfo()
    info.width, info.height = w, h
    info.n_comp, info.n_qtabs = 3, 1
    cw, ch = (w if sampling == 444 else w // 2), (h // 2 if sampling == 420 else h)
    po = 0
    for i, (hs, vs) in enumerate(FACTORS[sampling]):
        info.comp[i].hscale, info.comp[i].vscale = hs, vs
        pw, ph = (w, h) if i == 0 else (cw, ch)
        L = info.layout[i]
        L.stride = pw + pad_w
        L.coef_offset, L.plane_offset = po, po
        po += L.stride * ph
    info.coef_count, info.pixel_bytes = po, po
    return info


FIELDS = ("frame", "y_base", "cb_base", "cr_base", "rgb_base", "y_stride", "cb_stride", "cr_stride", "row_stride", "plane_stride",
          "w", "h", "cw", "ch", "sampling", "vec_y", "vec_c", "vec_rgb", "groups", "magic", "lanes", "unit0")


def run_builder(harness, tmp_path, infos, yuv_offsets, rgb_offsets, strides=None, layout=0, frames=None, yuv_addr=0, rgb_addr=0):
    n = len(infos)
    raw = struct.pack("<6q", n, -1 if frames is None else len(frames), layout, yuv_addr, rgb_addr, int(strides is not None))
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


def place(infos, align=256):
    yuv, rgb, yo, ro = [], [], 0, 0
    for i in infos:
        yuv.append(yo)
        rgb.append(ro)
        yo += -(-i.pixel_bytes // 64) * 64
        ro += -(-(3 * i.width * i.height) // align) * align
    return yuv, rgb


def check_lanes(plan):
    """every lane of every image in exactly one (unit, lane), by the kernel's own arithmetic; units contiguous, every unit names
    the image that owns it"""
    want_map = []
    for i, k in enumerate(plan["images"]):
        assert k["unit0"] == len(want_map)
        want_map += [i] * (-(-k["lanes"] // 64))
    assert plan["map"] == want_map
    for i, k in enumerate(plan["images"]):
        lrows = k["lanes"] // k["groups"]
        seen = np.zeros((lrows, k["groups"]), dtype=int)
        assert k["magic"] == (0 if k["groups"] == 1 else -(-(1 << 32) // k["groups"]))
        for u in [u for u, x in enumerate(plan["map"]) if x == i]:
            for lane in range(64):
                t = (u - k["unit0"]) * 64 + lane
                if t < k["lanes"]:
                    lr = t if k["groups"] == 1 else (t * k["magic"]) >> 32
                    assert lr == t // k["groups"]
                    seen[lr, t - lr * k["groups"]] += 1
        assert (seen == 1).all(), i


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_the_geometries_of_the_gpu_suite(hvc, harness, tmp_path, order):
    geo = GEOMETRIES if order == "forward" else GEOMETRIES[::-1]
    infos = [hvc.jpeg_encoder_layout(w, h, s, 75) for s, w, h, _ in geo]
    yuv, rgb = place(infos)
    plan = run_builder(harness, tmp_path, infos, yuv, rgb)
    assert plan["status"] == 0 and plan["check"] == "ok"
    im = plan["images"]
    assert [k["frame"] for k in im] == list(range(len(geo)))
    assert [k["lanes"] for k in im] == [g[3] for g in geo]
    assert [k["sampling"] for k in im] == [g[0] for g in geo]
    assert [k["groups"] for k in im] == [-(-g[1] // 8) for g in geo]
    assert [(k["cw"], k["ch"]) for k in im] == [(w if s == 444 else w // 2, h // 2 if s == 420 else h) for s, w, h, _ in geo]
    assert plan["lanes"] == sum(g[3] for g in geo)
    check_lanes(plan)
    assert len(plan["map"]) == sum(-(-g[3] // 64) for g in geo) == 22 and len(plan["map"]) % 4 != 0    # the last workgroup has spare units
    # bases: the frame's offset plus the plane's; the padded planes of the encoder's layout take the 8-byte paths
    for f, k in enumerate(im):
        assert k["y_base"] == yuv[f] and k["cb_base"] == yuv[f] + infos[f].layout[1].plane_offset
        assert k["cr_base"] == yuv[f] + infos[f].layout[2].plane_offset and k["rgb_base"] == rgb[f]
        assert (k["y_stride"], k["cb_stride"]) == (infos[f].layout[0].stride, infos[f].layout[1].stride)
        assert k["row_stride"] == 3 * k["w"] and (k["vec_y"], k["vec_c"]) == (1, 1)
        assert k["vec_rgb"] == int(3 * k["w"] % 8 == 0)


def test_the_lane_count_is_the_encoders_not_the_decoders(hvc, harness, tmp_path):
    """h / 2 lane rows and w / 2 chroma samples: a 4:2:0 frame of 64 x 16 has 8 x 8 lanes, as in the decode direction, but one
    of 40 x 26 has 5 x 13 either way while 6 x 4 has 2 lanes here; 257 rows of one lane; 257 lanes in one row"""
    infos = [raw_image(hvc, 64, 16, 420), raw_image(hvc, 40, 26, 420), raw_image(hvc, 6, 4, 420), raw_image(hvc, 7, 257, 444),
             raw_image(hvc, 2050, 1, 422), raw_image(hvc, 128, 16, 422)]
    yuv, rgb = place(infos)
    plan = run_builder(harness, tmp_path, infos, yuv, rgb)
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert [k["lanes"] for k in plan["images"]] == [64, 65, 2, 257, 257, 256]
    assert [k["groups"] for k in plan["images"]] == [8, 5, 1, 1, 257, 16]
    check_lanes(plan)


def test_an_empty_set_only_refused_frames_and_a_list_with_holes(hvc, harness, tmp_path):
    none = run_builder(harness, tmp_path, [], [], [])
    assert none["status"] == 0 and none["images"] == [] and none["map"] == [] and none["lanes"] == 0
    odd = [raw_image(hvc, 7, 4, 420), raw_image(hvc, 8, 3, 420), raw_image(hvc, 9, 3, 422)]
    for k in range(3):
        bad = run_builder(harness, tmp_path, odd[k:], [0, 4096, 8192][k:], [0, 4096, 8192][k:])
        assert bad["status"] == -1 and "check" not in bad                                       # (no table left behind)
    infos = [raw_image(hvc, 16, 16, 420), odd[0], raw_image(hvc, 600, 3, 444), odd[2], raw_image(hvc, 24, 24, 422)]
    yuv, rgb = place(infos)
    assert run_builder(harness, tmp_path, infos, yuv, rgb)["status"] == -1                      # the whole plan
    plan = run_builder(harness, tmp_path, infos, yuv, rgb, frames=[4, 0, 2])                    # a list, not a range
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert [k["frame"] for k in plan["images"]] == [4, 0, 2] and [k["lanes"] for k in plan["images"]] == [72, 16, 225]
    assert plan["map"] == [0, 0, 1, 2, 2, 2, 2] and plan["images"][0]["y_base"] == yuv[4] and plan["images"][1]["rgb_base"] == 0
    check_lanes(plan)
    assert run_builder(harness, tmp_path, infos, yuv, rgb, frames=[4, 1])["status"] == -1
    assert run_builder(harness, tmp_path, infos, yuv, rgb, frames=[])["images"] == []
    # a frame without a pixel gets no descriptor
    plan = run_builder(harness, tmp_path, [raw_image(hvc, 16, 0, 422), raw_image(hvc, 16, 2, 422)], [0, 64], [0, 64])
    assert plan["status"] == 0 and [k["frame"] for k in plan["images"]] == [1]


@pytest.mark.parametrize("m", [0, 1, 4, 8])
def test_flags_follow_the_actual_bases_and_strides(hvc, harness, tmp_path, m):
    """bases and strides at 0, 1, 4 and 8 modulo 8: offsets, the addresses they count from, and the row strides"""
    def flags(plan):
        return [(k["vec_y"], k["vec_c"], k["vec_rgb"]) for k in plan["images"]]
    on8, on4 = int(m % 8 == 0), int(m % 4 == 0)
    infos = [raw_image(hvc, 64, 16, 420), raw_image(hvc, 64, 16, 422), raw_image(hvc, 64, 16, 444)]
    base = [0, 8192, 16384]
    # the record's offset: luma and the image want 8, the chroma of 4:2:0 / 4:2:2 wants 4, of 4:4:4 8
    plan = run_builder(harness, tmp_path, infos, [b + m for b in base], base)
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert flags(plan) == [(on8, on4, 1), (on8, on4, 1), (on8, on8, 1)]
    plan = run_builder(harness, tmp_path, infos, base, [b + m for b in base])
    assert flags(plan) == [(1, 1, on8)] * 3
    # the addresses the offsets count from are part of it
    plan = run_builder(harness, tmp_path, infos, base, base, yuv_addr=0x7000000 + m, rgb_addr=0x9000000)
    assert flags(plan) == [(on8, on4, 1), (on8, on4, 1), (on8, on8, 1)]
    plan = run_builder(harness, tmp_path, infos, base, base, yuv_addr=0x7000000, rgb_addr=0x9000000 + m)
    assert flags(plan) == [(1, 1, on8)] * 3 and plan["check"] == "ok"
    # plane strides: width + m (luma 64 + m, chroma 32 + m or 64 + m); the planes follow one another, so the bases move too
    padded = [raw_image(hvc, 64, 16, s, pad_w=m) for s in (420, 422, 444)]
    plan = run_builder(harness, tmp_path, padded, base, base)
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert flags(plan) == [(on8, on4, 1), (on8, on4, 1), (on8, on8, 1)]
    # RGB row strides: tight + m; planar planes also need row_stride * h on 8 (h = 16: always)
    plan = run_builder(harness, tmp_path, infos, base, base, strides=[192 + m] * 3)
    assert flags(plan) == [(1, 1, on8)] * 3
    plan = run_builder(harness, tmp_path, infos, base, base, strides=[64 + m] * 3, layout=1)
    assert flags(plan) == [(1, 1, on8)] * 3 and plan["images"][0]["plane_stride"] == (64 + m) * 16
    tall = raw_image(hvc, 12, 3, 444)                                                           # 3 rows of 12: planes 36 apart
    plan = run_builder(harness, tmp_path, [tall], [0], [0], strides=[12 + m], layout=1)
    assert plan["images"][0]["vec_rgb"] == int((12 + m) % 8 == 0 and (12 + m) * 3 % 8 == 0) and plan["check"] == "ok"


def test_refusals(hvc, harness, tmp_path):
    ok = raw_image(hvc, 40, 24, 420)
    assert run_builder(harness, tmp_path, [ok], [0], [0])["status"] == 0
    assert run_builder(harness, tmp_path, [ok], [0], [0], layout=2)["status"] == -1             # a layout that is neither
    for s, w, h, want in ((420, 41, 24, -1), (422, 41, 24, -1), (444, 41, 25, 0), (420, 40, 25, -1), (422, 40, 25, 0)):
        assert run_builder(harness, tmp_path, [raw_image(hvc, w, h, s)], [0], [0])["status"] == want, (s, w, h)   # the even-size rule
    grey = raw_image(hvc, 40, 24, 444)
    grey.n_comp = 1
    assert run_builder(harness, tmp_path, [grey], [0], [0])["status"] == -1                     # monochrome is not encoded
    for fac in ([(4, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(2, 1), (1, 1)], [(2, 2), (1, 1), (1, 1), (2, 2)]):
        bad = raw_image(hvc, 40, 24, 444)
        bad.n_comp = len(fac)
        for i, (hs, vs) in enumerate(fac):
            bad.comp[i].hscale, bad.comp[i].vscale = hs, vs
        assert run_builder(harness, tmp_path, [ok, bad], [0, 4096], [0, 4096])["status"] == -1  # a sampling that is none of the three
        assert run_builder(harness, tmp_path, [ok, bad], [0, 4096], [0, 4096], frames=[0])["status"] == 0
    short = raw_image(hvc, 40, 24, 420)
    short.layout[0].stride = 39
    assert run_builder(harness, tmp_path, [short], [0], [0])["status"] == -1                    # a stride below its row
    short = raw_image(hvc, 40, 24, 420)
    short.layout[2].stride = 19
    assert run_builder(harness, tmp_path, [short], [0], [0])["status"] == -1
    assert run_builder(harness, tmp_path, [ok], [0], [0], strides=[119])["status"] == -1        # an RGB row stride below 3 w
    assert run_builder(harness, tmp_path, [ok], [0], [0], strides=[40], layout=1)["status"] == 0
    small = hvc.jpeg_encoder_layout(40, 24, 420, 75)
    small.layout[1].blocks_h = 1                                                                # 12 chroma rows in a plane of 8
    assert run_builder(harness, tmp_path, [small], [0], [0])["status"] == -1
    neg = raw_image(hvc, 40, 24, 420)
    neg.width = -2
    assert run_builder(harness, tmp_path, [neg], [0], [0])["status"] == -1                      # a negative size
    neg = raw_image(hvc, 40, 24, 444)
    neg.height = -1
    assert run_builder(harness, tmp_path, [neg], [0], [0])["status"] == -1
    # HVC_E_TOO_LARGE as in the decode plan: HVC_MIXED_MAX_UNITS = 2^26 units (an image of 2 x 2^24 lanes has 2^19 of them),
    # lanes * groups = 2^32, a side above 2^24
    tall = raw_image(hvc, 16, 1 << 24, 444)
    assert run_builder(harness, tmp_path, [tall], [0], [0], frames=[0] * 129)["status"] == -7
    wide = raw_image(hvc, 16384, 1024, 444)
    assert run_builder(harness, tmp_path, [wide], [0], [0])["status"] == -7
    assert run_builder(harness, tmp_path, [raw_image(hvc, 16384, 2046, 420)], [0], [0])["status"] == 0   # (1023 lane rows: just below)
    huge = raw_image(hvc, (1 << 24) + 2, 2, 420)
    assert run_builder(harness, tmp_path, [huge], [0], [0])["status"] == -7


def test_seeded_random_sets_in_the_sanitizer_build(harness):
    r = subprocess.run([harness, "random", "20261019", "400"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.split()[:2] == ["ok", "400"]
