"""The host plan of the resampling step over a mixed set (csrc/hvc_resize_plan.cpp), without a GPU, through the stand-alone
program tests/host_harness/resize_plan_harness.cpp -- which keeps the plan out of the public header and runs it under
AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only g++ build: tests/host_harness/Makefile.resize).  Every tap and
bound of the axis tables must equal tools/resize_reference.py as integers.  Nothing loaded into Python runs under a sanitizer."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import resize_reference as rr  # noqa: E402

HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
MAX_TAPS = 2048

N_IN = list(range(1, 71)) + [97, 255, 256, 257, 480, 1920, 4096]
N_OUT = [1, 2, 3, 8, 17, 31, 64, 100, 224, 257, 480, 1000]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resize") / "resize_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.resize", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def run(harness, *args):
    r = subprocess.run([harness] + [str(a) for a in args], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_tables_equal_the_definition_tap_for_tap(harness, tmp_path):
    """sizes 1 .. 70, 97, 255 .. 257, 480, 1920, 4096 against a dozen outputs under the three filters: xmin, count and every
    tap as integers; a position with more than 2048 taps refuses the table; the overflow check holds over the sweep"""
    out = tmp_path / "sweep.bin"
    said = run(harness, "sweep", out, *N_IN, "--", *N_OUT).split()
    assert said[0] == "ok" and int(said[1]) == len(N_IN) * len(N_OUT) * 3
    assert 255 * int(said[3]) + (1 << 21) < (1 << 31)
    raw = np.fromfile(str(out), dtype=np.int32)
    at, seen, refused, worst = 0, 0, 0, 0
    for n_in in N_IN:
        for n_out in N_OUT:
            for fi, f in enumerate(rr.FILTERS):
                head = raw[at:at + 5].tolist()
                at += 5
                xmin, count, taps = rr.coefficients(n_in, n_out, f)
                kmax = int(count.max())
                if kmax > MAX_TAPS:
                    assert head == [n_in, n_out, fi, -7, 0]
                    refused += 1
                    continue
                assert head == [n_in, n_out, fi, 0, kmax]
                got_xmin, got_count, got_first = (raw[at + i * n_out:at + (i + 1) * n_out] for i in range(3))
                at += 3 * n_out
                got_taps = raw[at:at + kmax * n_out].reshape(kmax, n_out)      # transposed: tap i of position p at [i, p]
                at += kmax * n_out
                assert np.array_equal(got_xmin, xmin) and np.array_equal(got_count, count), (n_in, n_out, f)
                assert np.array_equal(got_first, np.arange(n_out)), (n_in, n_out, f)
                assert np.array_equal(got_taps.T, taps), (n_in, n_out, f)
                assert np.abs(taps).max() < (1 << 23)
                worst = max(worst, int(np.abs(taps).sum(axis=1).max()))
                seen += 1
    assert at == raw.size and seen + refused == len(N_IN) * len(N_OUT) * 3
    assert refused == 7        # 4096 -> 1 under every filter, 4096 -> 2 and -> 3 under bilinear and bicubic: above 2048 taps
    assert worst == int(said[3]) == rr.max_abs_tap_sum(69, 64, "bicubic") == 5321270   # 1.269 * 2^22, as the header says


def test_one_axis_of_each_kind_by_hand():
    """the definition on cases small enough to check by eye"""
    xmin, count, taps = rr.coefficients(4, 2, "box")
    assert xmin.tolist() == [0, 2] and count.tolist() == [2, 2] and taps.tolist() == [[1 << 21, 1 << 21]] * 2
    xmin, count, taps = rr.coefficients(5, 5, "bicubic")                       # the identity, whatever the filter
    assert [int(taps[p, :count[p]] @ (np.arange(xmin[p], xmin[p] + count[p]) == p)) for p in range(5)] == [1 << 22] * 5
    xmin, count, taps = rr.coefficients(3, 3, "box")
    assert xmin.tolist() == [0, 1, 2] and count.tolist() == [1, 1, 1] and taps[:, 0].tolist() == [1 << 22] * 3


FIELDS = ("image", "src_base", "dst_base", "src_stride", "dst_stride", "rec0", "tap_stride", "n_out", "rows", "ch", "row_bytes", "groups",
          "magic", "lanes", "units", "unit0", "src_sel", "dst_sel", "vec")


def run_plan(harness, tmp_path, images, layout=0, filt=1, frames=None, src_addr=0, dst_addr=0):
    """images: (w, h, out_w, out_h, src_offset, src_row_stride, dst_offset, dst_row_stride)"""
    raw = struct.pack("<6q", len(images), -1 if frames is None else len(frames), layout, filt, src_addr, dst_addr)
    raw += b"".join(struct.pack("<8q", *im) for im in images)
    if frames is not None:
        raw += struct.pack("<%di" % len(frames), *frames)
    p = tmp_path / "set.bin"
    p.write_bytes(raw)
    out = dict(h=[], v=[], hmap=[], vmap=[], tables=[])
    for ln in run(harness, "plan", p).splitlines():
        w = ln.split()
        if w[0] in ("status", "mid", "empty"):
            out[w[0]] = int(w[1])
        elif w[0] == "check":
            out["check"] = " ".join(w[1:])
        elif w[0] == "words":
            out["words"] = (int(w[1]), int(w[2]))
        elif w[0] == "table":
            out["tables"].append(tuple(map(int, w[1:])))
        elif w[0] in ("h", "v"):
            out[w[0]].append(dict(zip(FIELDS, map(int, w[2:]))))
        elif w[0] in ("hmap", "vmap"):
            out[w[0]] = list(map(int, w[1:]))
    return out


def place(images, layout=0):
    """tight records one after another, each on 64 bytes"""
    out, so, do = [], 0, 0
    for w, h, ow, oh in images:
        out.append((w, h, ow, oh, so, 0, do, 0))
        so += -(-(3 * w * h) // 64) * 64
        do += -(-(3 * ow * oh) // 64) * 64
    return out


def test_descriptors_and_map_of_a_mixed_set(harness, tmp_path):
    """units of 1, 63, 64, 65 lanes and a workgroup's edge (255, 257) in both passes; a skipped axis gets no descriptor"""
    sizes = [
        (5, 1, 1, 1),        # h only: 1 lane
        (2, 3, 21, 3),       # h only: 63 lanes
        (10, 8, 8, 8),       # h only: 64
        (9, 13, 5, 13),      # h only: 65
        (97, 51, 5, 17),     # both: h 255 lanes; v rows of 15 bytes = 4 lanes
        (300, 1, 257, 1),    # h only: 257
        (1, 5, 1, 2),        # v only: rows of 3 bytes = 1 lane
        (84, 7, 84, 3),      # v only: 252 bytes = 63 lanes
        (85, 7, 85, 3),      # v only: 255 bytes = 64 lanes (the last takes the byte path)
        (86, 7, 86, 3),      # v only: 258 bytes = 65 lanes, two units per row
        (340, 4, 340, 2),    # v only: 1020 bytes = 255 lanes
        (342, 4, 342, 2),    # v only: 1026 bytes = 257 lanes, five units per row
        (17, 9, 17, 9),      # the copy: vertical, identity table
    ]
    plan = run_plan(harness, tmp_path, place(sizes), filt=2)
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert [k["image"] for k in plan["h"]] == [0, 1, 2, 3, 4, 5]
    assert [k["lanes"] for k in plan["h"]] == [1, 63, 64, 65, 255, 257]
    assert [k["units"] for k in plan["h"]] == [1, 1, 1, 2, 4, 5]
    assert [k["image"] for k in plan["v"]] == [4, 6, 7, 8, 9, 10, 11, 12]
    assert [k["lanes"] for k in plan["v"]] == [4, 1, 63, 64, 65, 255, 257, 13]
    assert [k["groups"] for k in plan["v"]] == [1, 1, 1, 1, 2, 4, 5, 1]
    assert [k["units"] for k in plan["v"]] == [17, 2, 3, 3, 6, 8, 10, 9]
    for name in ("h", "v"):
        want = []
        for i, k in enumerate(plan[name]):
            assert k["unit0"] == len(want)
            want += [i] * k["units"]
        assert plan[name + "map"] == want
    # image 4 goes through the intermediate: rows of 15 bytes on 16, the vertical pass reads what the horizontal one wrote
    h4, v4 = plan["h"][4], plan["v"][0]
    assert (h4["dst_sel"], v4["src_sel"]) == (1, 1) and h4["dst_base"] == v4["src_base"] == 0 and h4["dst_stride"] == v4["src_stride"] == 16
    assert plan["mid"] == 16 * 51
    assert all(k["dst_sel"] == 0 for i, k in enumerate(plan["h"]) if i != 4) and all(k["src_sel"] == 0 for k in plan["v"][1:])
    # tables: one per distinct (n_in, n_out, filter); the copy takes box 9 -> 9
    assert (9, 9, 0) in [t[:3] for t in plan["tables"]] and len(set(t[:3] for t in plan["tables"])) == len(plan["tables"])
    assert plan["h"][4]["tap_stride"] == 5


def test_tables_are_shared_and_planar_images_are_three(harness, tmp_path):
    sizes = [(64, 48, 24, 16), (64, 48, 24, 16), (48, 64, 16, 24), (64, 30, 24, 16)]
    plan = run_plan(harness, tmp_path, place(sizes), layout=1, filt=1)
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert sorted(t[:3] for t in plan["tables"]) == [(30, 16, 1), (48, 16, 1), (64, 24, 1)]
    assert len(plan["h"]) == len(plan["v"]) == 12 and [k["image"] for k in plan["h"]] == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert all(k["ch"] == 1 for k in plan["h"])
    # the planes of image 0: width x height apart in the source, out_w x out_h apart in the destination, never overlapping in between
    h0, v0 = plan["h"][:3], plan["v"][:3]
    assert [k["src_base"] for k in h0] == [0, 64 * 48, 2 * 64 * 48] and [k["dst_base"] for k in v0] == [0, 24 * 16, 2 * 24 * 16]
    assert [k["dst_base"] for k in h0] == [k["src_base"] for k in v0] == [0, 24 * 48, 2 * 24 * 48]
    # 64 -> 24 serves images 0, 1 and 3 horizontally and image 2 vertically: one table
    assert plan["h"][0]["rec0"] == plan["h"][3]["rec0"] == plan["h"][9]["rec0"] == plan["v"][6]["rec0"]


def test_the_dword_flag_follows_the_actual_addresses(harness, tmp_path):
    ims = [(40, 8, 40, 4, 0, 0, 0, 0), (40, 8, 40, 4, 4001, 121, 4000, 0), (40, 8, 40, 4, 8000, 124, 8000, 124), (41, 8, 41, 4, 12000, 0, 12000, 0),
           (41, 8, 20, 4, 16001, 0, 16000, 64)]
    plan = run_plan(harness, tmp_path, ims)
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert [k["vec"] for k in plan["v"]] == [1, 0, 1, 0, 1]      # (the last reads the intermediate: the odd source does not matter)
    plan = run_plan(harness, tmp_path, ims, src_addr=0x7000002)
    assert [k["vec"] for k in plan["v"]] == [0, 0, 0, 0, 1]
    plan = run_plan(harness, tmp_path, ims, dst_addr=0x7000001)
    assert [k["vec"] for k in plan["v"]] == [0, 0, 0, 0, 0]


def test_a_list_leaves_the_others_out(harness, tmp_path):
    ims = place([(16, 16, 8, 8), (0, 5, 8, 8), (24, 24, 8, 8)])
    plan = run_plan(harness, tmp_path, ims, frames=[2, 0])
    assert plan["status"] == 0 and plan["check"] == "ok" and [k["image"] for k in plan["h"]] == [2, 0]
    none = run_plan(harness, tmp_path, ims, frames=[])
    assert none["status"] == 0 and none["h"] == none["v"] == [] and none["mid"] == 0 and none["words"] == (0, 0)
    assert run_plan(harness, tmp_path, ims)["status"] == -1       # the image of width 0, listed


def test_refusals(harness, tmp_path):
    ok = (40, 24, 20, 12, 0, 0, 0, 0)
    assert run_plan(harness, tmp_path, [ok])["status"] == 0
    for filt in (-1, 3, 4):
        bad = run_plan(harness, tmp_path, [ok], filt=filt)
        assert bad["status"] == -1 and bad["empty"] == 1          # an unknown filter
    assert run_plan(harness, tmp_path, [ok], layout=2)["status"] == -1
    for i in range(4):                                            # a size below 1
        for v in (0, -3):
            im = list(ok)
            im[i] = v
            assert run_plan(harness, tmp_path, [ok, tuple(im)])["status"] == -1
    assert run_plan(harness, tmp_path, [(40, 24, 20, 12, 0, 119, 0, 0)])["status"] == -1      # a stride below the row
    assert run_plan(harness, tmp_path, [(40, 24, 20, 12, 0, 0, 0, 59)])["status"] == -1
    assert run_plan(harness, tmp_path, [(40, 24, 20, 12, 0, 40, 0, 20)], layout=1)["status"] == 0
    assert run_plan(harness, tmp_path, [(40, 24, 20, 12, 0, 39, 0, 20)], layout=1)["status"] == -1
    # the table bound: 2048 taps at a position
    assert run_plan(harness, tmp_path, [(2048, 1, 1, 1, 0, 0, 0, 0)], filt=0)["status"] == 0
    big = run_plan(harness, tmp_path, [ok, (2049, 1, 1, 1, 0, 0, 0, 0)], filt=0)
    assert big["status"] == -7 and big["empty"] == 1
    assert run_plan(harness, tmp_path, [(1, 8192, 1, 1, 0, 0, 0, 0)], filt=2)["status"] == -7   # 8192 -> 1 bicubic
    assert run_plan(harness, tmp_path, [(1025, 1, 1, 1, 0, 0, 0, 0)], filt=2)["status"] == 0
    # beyond 32-bit indices: a side above 2^24, lanes beyond the magic division (out_w * h * out_w >= 2^32)
    assert run_plan(harness, tmp_path, [((1 << 24) + 1, 1, 8, 1, 0, 0, 0, 0)])["status"] == -7
    assert run_plan(harness, tmp_path, [(8, 1, (1 << 24) + 1, 1, 0, 0, 0, 0)])["status"] == -7
    assert run_plan(harness, tmp_path, [(2049, 1024, 2048, 1024, 0, 0, 0, 0)])["status"] == -7
    assert run_plan(harness, tmp_path, [(2049, 1023, 2048, 1023, 0, 0, 0, 0)])["status"] == 0
    # the per-image verdict the file pipeline uses
    assert run(harness, "status", 480, 320, 1, 1, 2).split() == ["status", "0"]
    assert run(harness, "status", 4097, 1, 1, 1, 0).split() == ["status", "-7"]
    assert run(harness, "status", 40, 0, 8, 8, 1).split() == ["status", "-1"]
    assert run(harness, "status", 40, 8, 8, 8, 7).split() == ["status", "-1"]


def test_seeded_random_sets_in_the_sanitizer_build(harness):
    assert run(harness, "random", "20261020", "400").split()[:2] == ["ok", "400"]
