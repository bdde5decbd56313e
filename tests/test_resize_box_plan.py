"""The box / mirror / typed forms of the resampling plan (csrc/hvc_resize_plan.cpp: resize_axis_build_box,
resize_image_status_box, resize_plan_build_opts), without a GPU, through the stand-alone program
tests/host_harness/resize_box_plan_harness.cpp -- its own main, built under AddressSanitizer and UndefinedBehaviorSanitizer
(a CPU-only g++ build: tests/host_harness/Makefile.resize_box) and run as a program.  Every record and tap must equal tools/resize_reference.py
coefficients_box as integers.  Nothing loaded into Python runs under a sanitizer."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import resize_box_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resize_reference as rr  # noqa: E402

HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
E_INVALID_ARG, E_TOO_LARGE = -1, -7


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resize_box") / "resize_box_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.resize_box", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def bits(v):
    return struct.unpack("<i", struct.pack("<f", float(np.float32(v))))[0]


def ubits(v):
    return bits(v) & 0xFFFFFFFF


def want_table(n_in, n_out, f, in0, in1, reversed_=False, shift=0):
    """(xmin - shift, count, taps[n_out][kmax]) of the numpy form, in reverse output order under a mirror"""
    xmin, count, taps = rr.coefficients_box(n_in, n_out, f, in0, in1)
    if reversed_:
        xmin, count, taps = xmin[::-1], count[::-1], taps[::-1]
    return xmin - shift, count, taps


def run_axes(harness, tmp_path, axes):
    """axes: (n_in, n_out, filter index, in0, in1, reversed, shift) -> per axis (status, xmin, count, first, taps[kmax][n_out])"""
    p, out = tmp_path / "axes.bin", tmp_path / "axes.out"
    p.write_bytes(b"".join(struct.pack("<7i", a[0], a[1], a[2], bits(a[3]), bits(a[4]), int(a[5]), a[6]) for a in axes))
    assert run(harness, "axes", p, out).split() == ["ok", str(len(axes))]
    raw = np.fromfile(str(out), dtype=np.int32)
    at, res = 0, []
    for a in axes:
        status, kmax = raw[at:at + 2].tolist()
        at += 2
        if status:
            res.append((status, None, None, None, None))
            continue
        n_out = a[1]
        cols = [raw[at + i * n_out:at + (i + 1) * n_out] for i in range(3)]
        at += 3 * n_out
        res.append((0, cols[0], cols[1], cols[2], raw[at:at + kmax * n_out].reshape(kmax, n_out)))
        at += kmax * n_out
    assert at == raw.size
    return res


def test_every_record_and_tap_equals_the_numpy_form(harness, tmp_path):
    """sizes 1 .. 70 to 1 .. 2 w under the three filters and every kind of box of tests/resize_box_cases.py, on both axes of the
    image, forwards and reversed, unshifted and shifted by xmin[0]; and the axis whose span differs between single and double"""
    axes = [(51, 14, 2, 4.75789737701416, 24.519044876098633, False, 0)]
    for w, h in bc.IN_SIZES:
        for bname, box in bc.boxes(w, h).items():
            x0, y0, x1, y1 = box if box is not None else (0.0, 0.0, float(w), float(h))
            for n_in, lo, hi in ((w, x0, x1), (h, y0, y1)):
                for n_out in sorted({1, 3, 8, 17, n_in, 2 * n_in}):
                    for fi, f in enumerate(rr.FILTERS):
                        first = rr.row_window(n_in, n_out, f, lo, hi)[0]
                        axes.append((n_in, n_out, fi, lo, hi, False, 0))
                        axes.append((n_in, n_out, fi, lo, hi, True, 0))
                        axes.append((n_in, n_out, fi, lo, hi, False, first))
    assert len(axes) > 2500
    got = run_axes(harness, tmp_path, axes)
    shifted = 0
    for a, (status, xmin, count, first, taps) in zip(axes, got):
        assert status == 0, a
        w_xmin, w_count, w_taps = want_table(a[0], a[1], rr.FILTERS[a[2]], a[3], a[4], a[5], a[6])
        assert np.array_equal(xmin, w_xmin) and np.array_equal(count, w_count), a
        assert np.array_equal(first, np.arange(a[1])), a
        assert taps.shape[0] == w_taps.shape[1] and np.array_equal(taps.T, w_taps), a
        shifted += a[6] > 0
    assert shifted > 100                                          # (boxes away from the top: the shift is not always 0)


def test_the_whole_window_is_the_axis_without_one(harness, tmp_path):
    axes = [(n_in, n_out, fi, 0.0, float(n_in), False, 0) for n_in in (1, 2, 17, 69, 480) for n_out in (1, 8, 64, 100) for fi in range(3)]
    for a, (status, xmin, count, first, taps) in zip(axes, run_axes(harness, tmp_path, axes)):
        w_xmin, w_count, w_taps = rr.coefficients(a[0], a[1], rr.FILTERS[a[2]])
        assert status == 0 and np.array_equal(xmin, w_xmin) and np.array_equal(count, w_count) and np.array_equal(taps.T, w_taps), a


def test_axis_refusals_and_bounds(harness, tmp_path):
    nan, inf = float("nan"), float("inf")
    bad = [(17, 8, 1, nan, 9.0), (17, 8, 1, 0.0, nan), (17, 8, 1, 0.0, inf), (17, 8, 1, -inf, 9.0),          # a non-finite value
           (17, 8, 1, -0.25, 9.0), (17, 8, 1, 0.0, 17.5),                                                    # leaving the samples
           (17, 8, 1, 5.0, 5.0), (17, 8, 1, 6.0, 5.0),                                                       # a span of 0 (Pillow lets it through), below 0
           (17, 8, 1, 16777216.0, 16777216.0)]
    got = run_axes(harness, tmp_path, [b + (False, 0) for b in bad] + [(17, 8, 1, -0.0, 17.0, False, 0), (17, 8, 3, 0.0, 17.0, False, 0)])
    assert [g[0] for g in got] == [E_INVALID_ARG] * len(bad) + [0, E_INVALID_ARG]
    # the bounds are the ones without a box: 2048 taps at a position, per position, whatever the window
    got = run_axes(harness, tmp_path, [(4096, 1, 0, 0.0, 2048.0, False, 0), (4096, 1, 0, 0.0, 2049.0, False, 0), (4096, 1, 0, 1000.5, 3048.5, False, 0),
                                       (4096, 1, 0, 1000.5, 3049.5, False, 0), (8192, 1, 2, 0.0, 8192.0, False, 0), ((1 << 24) + 1, 8, 1, 0.0, 8.0, False, 0),
                                       (4096, 2, 2, 0.0, 1024.0, False, 0), (17, 8, 1, 4.0, 9.0, False, 5)])
    assert [g[0] for g in got[:7]] == [0, E_TOO_LARGE, 0, E_TOO_LARGE, E_TOO_LARGE, E_TOO_LARGE, 0]
    assert got[7][0] != 0                                         # a shift above the smallest xmin is no table
    assert int(got[0][2].max()) == 2048


FIELDS = ("image", "src_base", "dst_base", "src_stride", "dst_stride", "rec0", "tap_stride", "n_out", "rows", "ch", "row_bytes", "groups",
          "magic", "lanes", "units", "unit0", "src_sel", "dst_sel", "vec", "dvec", "chan")
TABLE = ("n_in", "n_out", "filter", "rec0", "in0_bits", "in1_bits", "mirrored", "shift")


def run_plan(harness, tmp_path, images, layout=0, filt=1, frames=None, src_addr=0, dst_addr=0, boxes=None, mirror=None, out_elem=0):
    """images: (w, h, out_w, out_h, src_offset, src_row_stride, dst_offset, dst_row_stride); boxes: one (x0, y0, x1, y1) or None
    (the whole image) per image, or None for no boxes at all; mirror: one flag per image, or None"""
    n = len(images)
    raw = struct.pack("<9q", n, -1 if frames is None else len(frames), layout, filt, src_addr, dst_addr, boxes is not None, mirror is not None, out_elem)
    for i, im in enumerate(images):
        b = boxes[i] if boxes is not None and boxes[i] is not None else (0.0, 0.0, float(im[0]), float(im[1]))
        raw += struct.pack("<9q", *im, int(bool(mirror[i])) if mirror is not None else 0) + struct.pack("<4f", *b) + bytes(8)
    if frames is not None:
        raw += struct.pack("<%di" % len(frames), *frames)
    p, tab = tmp_path / "set.bin", tmp_path / "tables.bin"
    p.write_bytes(raw)
    out = dict(h=[], v=[], hmap=[], vmap=[], tables=[])
    for ln in run(harness, "plan", p, tab).splitlines():
        w = ln.split()
        if w[0] in ("status", "mid", "empty"):
            out[w[0]] = int(w[1])
        elif w[0] == "check":
            out["check"] = " ".join(w[1:])
        elif w[0] == "words":
            out["words"] = (int(w[1]), int(w[2]))
        elif w[0] == "table":
            out["tables"].append(dict(zip(TABLE, map(int, w[1:]))))
        elif w[0] in ("h", "v"):
            out[w[0]].append(dict(zip(FIELDS, map(int, w[2:]))))
        elif w[0] in ("hmap", "vmap"):
            out[w[0]] = list(map(int, w[1:]))
    if out["status"] == 0:
        raw = np.fromfile(str(tab), dtype=np.int32)
        n_recs, n_taps = raw[:2].tolist()
        out["recs"] = raw[2:2 + 3 * n_recs].reshape(n_recs, 3)
        out["taps"] = raw[2 + 3 * n_recs:]
        assert out["taps"].size == n_taps == out["words"][1] and n_recs == out["words"][0]
    return out


def table_of(plan, k):
    """(xmin, count, taps[n_out][kmax]) of descriptor k's table as the kernels read it: record p at rec0 + p, tap i at first + i * tap_stride"""
    n_out, rec0 = k["n_out"], k["rec0"]
    recs = plan["recs"][rec0:rec0 + n_out]
    kmax = int(recs[:, 1].max())
    taps = np.zeros((n_out, kmax), dtype=np.int64)
    for p in range(n_out):
        for i in range(recs[p, 1]):
            taps[p, i] = plan["taps"][recs[p, 2] + i * k["tap_stride"]]
    return recs[:, 0], recs[:, 1], taps


def place(images, layout=0, elem=1):
    out, so, do = [], 0, 0
    for w, h, ow, oh in images:
        out.append((w, h, ow, oh, so, 0, do, 0))
        so += -(-(3 * w * h) // 64) * 64
        do += -(-(3 * ow * oh * elem) // 64) * 64
    return out


SIZES = [(53, 45, 31, 17), (53, 45, 53, 45), (17, 9, 34, 18), (64, 48, 64, 16), (64, 48, 24, 48), (70, 53, 8, 8), (5, 7, 5, 7)]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("filt", [0, 1, 2])
def test_plan_under_boxes_and_mirrors(harness, tmp_path, filt, layout):
    """the row window of the horizontal pass, the shifted vertical records, the reversed records under a mirror, every table the
    numpy form's, mid_bytes the windows'"""
    f = rr.FILTERS[filt]
    kinds = ["fraction", "integer", "none", "bottom", "top", "thin", "whole"]
    boxes = [bc.boxes(w, h).get(kinds[i]) for i, (w, h, _, _) in enumerate(SIZES)]
    mirror = [1, 1, 0, 1, 0, 0, 1]
    plan = run_plan(harness, tmp_path, place(SIZES, layout), layout=layout, filt=filt, boxes=boxes, mirror=mirror)
    assert plan["status"] == 0 and plan["check"] == "ok"
    planes = 3 if layout else 1
    hk, vk = {k["image"]: k for k in plan["h"][::-1]}, {k["image"]: k for k in plan["v"][::-1]}   # (plane 0 of every image)
    mid = 0
    for i, (w, h, W, H) in enumerate(SIZES):
        x0, y0, x1, y1 = boxes[i] if boxes[i] is not None else (0.0, 0.0, float(w), float(h))
        skip_h, skip_v = rr.axis_skipped(w, W, x0, x1), rr.axis_skipped(h, H, y0, y1)
        need_h = not skip_h or bool(mirror[i])
        need_v = not skip_v or not need_h
        assert (i in hk) == need_h and (i in vk) == need_v, i
        row = W * (1 if layout else 3)
        ss = w * (1 if layout else 3)
        lo, hi = rr.row_window(h, H, "box" if skip_v else f, y0, y1) if need_v else (0, h)
        if need_h:
            k = hk[i]
            got = table_of(plan, k)
            want = want_table(w, W, "box" if skip_h else f, x0, x1, bool(mirror[i]))
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), i
            if need_v:      # only the rows the vertical pass reads
                assert k["rows"] == hi - lo and k["lanes"] == W * (hi - lo) and k["src_base"] == SIZES_OFF(plan, i, layout) + lo * ss, i
                assert k["dst_sel"] == 1
            else:
                assert k["rows"] == h and k["dst_sel"] == 0
        if need_v:
            k = vk[i]
            got = table_of(plan, k)
            want = want_table(h, H, "box" if skip_v else f, y0, y1, False, lo)           # shifted by ymin[0]
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), i
            assert got[0][0] == 0 and k["rows"] == (hi - lo if need_h else h - lo)
            if need_h:
                assert k["src_sel"] == 1 and k["src_base"] == hk[i]["dst_base"] and k["src_stride"] == hk[i]["dst_stride"] == -(-row // 4) * 4
                mid = -(-mid // 64) * 64 + k["src_stride"] * (hi - lo) * planes
            else:
                assert k["src_sel"] == 0 and k["src_base"] == SIZES_OFF(plan, i, layout) + lo * ss
        assert (k["dvec"], k["chan"]) == (0, 0)
    assert plan["mid"] == mid
    # image 1 (the same size, an integer box): both axes run; image 6 (the same size, the whole box, mirrored): the identity
    # table box 5 -> 5 reversed, and no vertical pass
    assert 1 in hk and 1 in vk and 6 in hk and 6 not in vk
    xmin, count, taps = table_of(plan, hk[6])
    assert xmin.tolist() == [4, 3, 2, 1, 0] and count.tolist() == [1] * 5 and taps[:, 0].tolist() == [1 << 22] * 5
    keys = [(t["n_in"], t["n_out"], t["filter"], t["in0_bits"], t["in1_bits"], t["mirrored"], t["shift"]) for t in plan["tables"]]
    assert len(set(keys)) == len(keys)
    assert (5, 5, 0, 0, ubits(5.0), 1, 0) in keys


def SIZES_OFF(plan, i, layout):
    return place(SIZES, layout)[i][4]


def test_tables_are_shared_by_the_new_key(harness, tmp_path):
    box, other = (3.5, 2.25, 40.0, 30.5), (3.5, 2.25, 40.0, 30.75)
    sizes = [(64, 48, 24, 16)] * 5
    plan = run_plan(harness, tmp_path, place(sizes), boxes=[box, box, other, box, None], mirror=[0, 0, 0, 1, 0])
    assert plan["status"] == 0 and plan["check"] == "ok"
    h, v = plan["h"], plan["v"]
    assert h[0]["rec0"] == h[1]["rec0"] == h[2]["rec0"] and v[0]["rec0"] == v[1]["rec0"] == v[3]["rec0"]      # the same key: one table
    assert h[3]["rec0"] != h[0]["rec0"]                           # mirrored: another table
    assert v[2]["rec0"] != v[0]["rec0"]                           # one bit of in1: another table
    assert len({h[4]["rec0"], h[0]["rec0"], v[4]["rec0"], v[0]["rec0"]}) == 4
    assert len(plan["tables"]) == 6
    want = {(64, 24, ubits(3.5), ubits(40.0), 0), (64, 24, ubits(3.5), ubits(40.0), 1), (48, 16, ubits(2.25), ubits(30.5), 0),
            (48, 16, ubits(2.25), ubits(30.75), 0), (64, 24, 0, ubits(64.0), 0), (48, 16, 0, ubits(48.0), 0)}
    assert {(t["n_in"], t["n_out"], t["in0_bits"], t["in1_bits"], t["mirrored"]) for t in plan["tables"]} == want
    # without options: the plan of resize_plan_build, shared as there
    plain = run_plan(harness, tmp_path, place(sizes))
    assert len(plain["tables"]) == 2 and all(t["shift"] == 0 and t["mirrored"] == 0 for t in plain["tables"])


@pytest.mark.parametrize("elem", [2, 4])
def test_typed_output_ends_every_image_in_the_vertical_pass(harness, tmp_path, elem):
    sizes = [(53, 45, 31, 45), (17, 9, 17, 9), (64, 48, 24, 16), (5, 7, 5, 7)]   # h only, the copy, both, the copy mirrored
    for layout in (0, 1):
        ims = place(sizes, layout, elem)
        plan = run_plan(harness, tmp_path, ims, layout=layout, filt=2, mirror=[0, 0, 0, 1], out_elem=elem)
        assert plan["status"] == 0 and plan["check"] == "ok"
        planes = 3 if layout else 1
        assert [k["image"] for k in plan["v"]] == [i for i in range(4) for _ in range(planes)]
        assert [k["image"] for k in plan["h"]] == [i for i in (0, 2, 3) for _ in range(planes)]
        assert all(k["dst_sel"] == 1 for k in plan["h"])                       # no horizontal pass writes the destination
        assert [k["chan"] for k in plan["v"]] == ([0, 1, 2] * 4 if layout else [3] * 4)
        v0 = plan["v"][0]                                                      # image 0: the vertical axis is skipped -- the identity table
        xmin, count, taps = table_of(plan, v0)
        assert xmin.tolist() == list(range(45)) and count.tolist() == [1] * 45 and taps[:, 0].tolist() == [1 << 22] * 45
        assert (45, 45, 0) in [(t["n_in"], t["n_out"], t["filter"]) for t in plan["tables"]]
        # rows: samples; the destination's strides and offsets: bytes of elem per sample
        for k in plan["v"]:
            W = sizes[k["image"]][2]
            assert k["row_bytes"] == W * (1 if layout else 3) and k["dst_stride"] == k["row_bytes"] * elem and k["lanes"] == -(-k["row_bytes"] // 4)
        if layout:
            assert [k["dst_base"] for k in plan["v"][:3]] == [0, 31 * 45 * elem, 2 * 31 * 45 * elem]
    # the two flags are judged apart: the source's dword loads, the destination's 4-element stores
    im = (40, 8, 40, 4)
    row = 120 * elem
    cases = [((0, 0, 0, 0), 0, 0, (1, 1)), ((0, 0, 0, 0), 0, 4 * elem, (1, 1)), ((0, 0, 0, 0), 0, 2 * elem, (1, 0)), ((0, 0, 0, 0), 2, 0, (0, 1)),
             ((0, 0, 0, row + elem), 0, 0, (1, 0)), ((0, 0, 0, row + 4 * elem), 0, 0, (1, 1)), ((4 * elem, 0, 0, 0), 0, 0, (1, 1)),
             ((0, 121, 0, 0), 0, 0, (0, 1)), ((0, 0, 3 * elem, 0), 0, 0, (1, 0))]
    for (so, sstr, do, dstr), sa, da, flags in cases:
        plan = run_plan(harness, tmp_path, [im + (so, sstr, do, dstr)], src_addr=0x7000000 + sa, dst_addr=0x7100000 + da, out_elem=elem)
        assert plan["status"] == 0 and plan["check"] == "ok"
        assert (plan["v"][0]["vec"], plan["v"][0]["dvec"]) == flags, (so, sstr, do, dstr, sa, da)


def test_plan_refusals_and_unchanged_bounds(harness, tmp_path):
    ok = (40, 24, 20, 12, 0, 0, 0, 0)
    nan, inf = float("nan"), float("inf")
    assert run_plan(harness, tmp_path, [ok], boxes=[(1.5, 2.0, 30.0, 20.5)])["status"] == 0
    for box in ((nan, 0, 40, 24), (0, nan, 40, 24), (0, 0, inf, 24), (0, 0, 40, -inf), (-1, 0, 40, 24), (0, -0.5, 40, 24), (0, 0, 40.5, 24), (0, 0, 40, 25),
                (7, 0, 7, 24), (8, 0, 7, 24), (0, 11, 40, 11), (0, 12, 40, 11)):
        bad = run_plan(harness, tmp_path, [ok, ok], boxes=[None, box])
        assert bad["status"] == E_INVALID_ARG and bad["empty"] == 1, box
        assert run_plan(harness, tmp_path, [ok, ok], boxes=[None, box], frames=[0])["status"] == 0    # not listed: not looked at
    for elem in (1, 3, 8, -2):
        assert run_plan(harness, tmp_path, [ok], out_elem=elem)["status"] == E_INVALID_ARG
    # typed rows: the stride is held against out_w * 3 * elem bytes
    assert run_plan(harness, tmp_path, [(40, 24, 20, 12, 0, 0, 0, 119)], out_elem=2)["status"] == E_INVALID_ARG
    assert run_plan(harness, tmp_path, [(40, 24, 20, 12, 0, 0, 0, 120)], out_elem=2)["status"] == 0
    assert run_plan(harness, tmp_path, [(40, 24, 20, 12, 0, 0, 0, 239)], out_elem=4)["status"] == E_INVALID_ARG
    assert run_plan(harness, tmp_path, [(40, 24, 20, 12, 0, 0, 0, 80)], layout=1, out_elem=4)["status"] == 0
    # the bounds stay: 2048 taps per position, whatever the window; 2^24 table words for the call -- with a box of its own every
    # image has tables of its own, so a set the un-boxed call plans is refused
    assert run_plan(harness, tmp_path, [(4096, 1, 1, 1, 0, 0, 0, 0)], filt=0, boxes=[(100.0, 0, 2148.0, 1)])["status"] == 0
    assert run_plan(harness, tmp_path, [(4096, 1, 1, 1, 0, 0, 0, 0)], filt=0, boxes=[(100.0, 0, 2149.0, 1)])["status"] == E_TOO_LARGE
    many = [(2048, 1, 2000, 1, i * 6144, 0, i * 6000, 0) for i in range(9)]
    assert run_plan(harness, tmp_path, many, filt=2)["status"] == 0
    boxed = run_plan(harness, tmp_path, many, filt=2, boxes=[(i / 8.0, 0, 2040.0, 1) for i in range(9)])
    assert boxed["status"] == 0 and len(boxed["tables"]) == 9                  # a table per image
    big = [(2048, 1, 2000, 1, i * 6144, 0, i * 6000, 0) for i in range(2000)]
    assert run_plan(harness, tmp_path, big, filt=2)["status"] == 0
    too = run_plan(harness, tmp_path, big, filt=2, boxes=[(i / 2048.0, 0, 2040.0, 1) for i in range(2000)])
    assert too["status"] == E_TOO_LARGE and too["empty"] == 1                  # 2000 tables of at least 5 x 2000 words > 2^24
    # the per-image verdict the file pipeline uses
    def status(w, h, W, H, f, mirror=0, box=None):
        return int(run(harness, "status", w, h, W, H, f, mirror, *([ubits(v) for v in box] if box else [])).split()[1])
    assert status(480, 320, 1, 1, 2) == 0 and status(4097, 1, 1, 1, 0) == E_TOO_LARGE and status(40, 0, 8, 8, 1) == E_INVALID_ARG
    assert status(4097, 1, 1, 1, 0, box=(10.0, 0.0, 2058.0, 1.0)) == 0         # the window's taps, not the image's
    assert status(40, 24, 8, 8, 1, box=(0.0, 0.0, 40.5, 24.0)) == E_INVALID_ARG
    assert status(40, 24, 8, 8, 1, box=(5.0, 3.0, 5.0, 24.0)) == E_INVALID_ARG
    assert status(40, 24, 8, 8, 1, 1, box=(5.0, 3.0, 5.5, 24.0)) == 0
    assert status(40, 24, 40, 24, 7, 1) == E_INVALID_ARG


def test_seeded_random_sets_in_the_sanitizer_build(harness):
    assert run(harness, "random", "20261021", "400").split()[:2] == ["ok", "400"]
