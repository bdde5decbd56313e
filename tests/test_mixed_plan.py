"""The host plan of a mixed batch (csrc/hvc_mixed_plan.cpp), without a GPU: hvc_jpeg_mixed_layout through the library, the
descriptor builder through the stand-alone program tests/host_harness/mixed_plan_harness.cpp -- which keeps the builder out
of the public header and runs it, and the layout call, under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only
g++ build: tests/host_harness/Makefile.mixed).  Nothing loaded into Python runs under a sanitizer."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import golden_bytes
from test_host_entropy import UNUSUAL_SAMPLINGS, unusual_sampling_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixed") / "mixed_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.mixed", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def files():
    """golden files and unusual samplings, with a truncated file and a progressive SOF in the middle"""
    mini = golden_bytes("mini.jpg")
    out = [mini, golden_bytes("Mouse480.jpg")]
    out += [unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 40, 24, 7 * si)[0] for si in (0, 3, 9)]
    out.append(mini[:100])                                    # no SOS: HVC_E_BAD_JPEG
    out.append(mini.replace(b"\xff\xc0", b"\xff\xc2", 1))     # SOF2: HVC_E_UNSUPPORTED_MARKER
    out += [unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 97, 51, 7 * si + 1)[0] for si in (1, 8, 11)]
    return out


def header_status(hvc, data):
    try:
        return 0, hvc.jpeg_read_header(data)
    except Exception as e:   # HvcError
        return e.code, None


@pytest.mark.parametrize("align", [8, 256, 0, 4096])
def test_layout_offsets(hvc, files, align):
    lay = hvc.jpeg_mixed_layout(files, align)
    a = align or 256
    end = 0
    assert [lay.status[f] for f in (5, 6)] == [-8, -9]
    for f, data in enumerate(files):
        st, info = header_status(hvc, data)
        assert lay.status[f] == st, f
        if st:
            continue
        got = lay.infos[f]
        assert bytes(got) == bytes(info)                       # the record hvc_jpeg_decode lays out
        off = lay.pixel_offsets[f]
        assert off % a == 0 and off >= end and off - end < a   # aligned, behind the last record, no more than the rounding apart
        end = off + info.pixel_bytes
    assert lay.total_bytes == end                              # exact: the failed files took no room


def test_layout_arguments(hvc, files):
    for bad in (12, 4, 1, 24):
        with pytest.raises(hvc.HvcError) as e:
            hvc.jpeg_mixed_layout(files, bad)
        assert e.value.code == -1
    one = hvc.jpeg_mixed_layout(files[:1])
    assert len(one) == 1 and one.status[0] == 0 and one.pixel_offsets[0] == 0 and one.total_bytes == one.infos[0].pixel_bytes
    only_bad = hvc.jpeg_mixed_layout(files[5:7], 8)
    assert list(only_bad.status) == [-8, -9] and only_bad.total_bytes == 0
    assert hvc.jpeg_mixed_layout([]).total_bytes == 0


def test_layout_in_the_sanitizer_build(hvc, harness, files, tmp_path):
    paths = []
    for k, f in enumerate(files):
        p = tmp_path / ("f%d.jpg" % k)
        p.write_bytes(f)
        paths.append(str(p))
    for align in (8, 256):
        r = subprocess.run([harness, "layout", str(align)] + paths, capture_output=True, text=True, env=ENV)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        lines = r.stdout.splitlines()
        lay = hvc.jpeg_mixed_layout(files, align)
        assert lines[0] == "status 0 total %d" % lay.total_bytes
        for f in range(len(files)):
            assert lines[1 + f] == "file %d %d %d %d" % (f, lay.status[f], lay.pixel_offsets[f],
                                                        0 if lay.status[f] else lay.infos[f].pixel_bytes)
    r = subprocess.run([harness, "layout", "12"] + paths, capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and r.stdout.split()[:2] == ["status", "-1"]


# ---------------------------------------------------------------------------
# the descriptor builder

def make_info(hvc, planes, tables):
    """planes: (blocks_w, blocks_h, qtab) each, tight records; tables: arrays of 64"""
    info = hvc.JpegInfo()
    info.n_comp, info.n_qtabs = len(planes), len(tables)
    for t, q in enumerate(tables):
        for k in range(64):
            info.qtabs[t][k] = int(q[k])
    co = po = 0
    for i, (bw, bh, qt) in enumerate(planes):
        L = info.layout[i]
        L.blocks_w, L.blocks_h, L.qtab, L.coef_offset, L.plane_offset, L.stride = bw, bh, qt, co, po, bw * 8
        co += bw * bh * 64
        po += bw * bh * 64
    info.coef_count, info.pixel_bytes = co, po
    return info


def run_builder(harness, tmp_path, infos, coef_offsets, pixel_offsets, frames=None):
    n = len(infos)
    raw = struct.pack("<qq", n, -1 if frames is None else len(frames)) + b"".join(bytes(i) for i in infos)
    raw += struct.pack("<%dQ" % n, *coef_offsets) + struct.pack("<%dQ" % n, *pixel_offsets)
    if frames is not None:
        raw += struct.pack("<%di" % len(frames), *frames)
    p = tmp_path / "set.bin"
    p.write_bytes(raw)
    r = subprocess.run([harness, "dump", str(p)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(planes=[], tables=[], map=[])
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "status":
            out["status"] = int(w[1])
        elif w[0] == "check":
            out["check"] = " ".join(w[1:])
        elif w[0] == "blocks":
            out["blocks"] = int(w[1])
        elif w[0] == "plane":
            out["planes"].append(dict(zip(("coef_base", "pix_base", "stride", "bw", "nblk", "magic", "table", "unit0"), map(int, w[2:]))))
        elif w[0] == "table":
            v = list(map(int, w[2:]))
            out["tables"].append(dict(wide=v[0], ethr=v[1], qt=v[2:66], qpair=v[66:98]))
        elif w[0] == "map":
            out["map"] = list(map(int, w[1:]))
    return out


Q_A = np.arange(1, 65)
Q_B = np.arange(64, 0, -1)
Q_WIDE = np.where(np.arange(64) == 9, 300, 3)


def test_every_block_has_exactly_one_unit_and_lane(hvc, harness, tmp_path):
    """planes of 1, 63, 64, 65, 256 and 257 blocks, bw == 1, an empty plane; equal tables shared, unequal ones not"""
    infos = [
        make_info(hvc, [(1, 1, 0)], [Q_A]),
        make_info(hvc, [(9, 7, 0), (8, 8, 1), (5, 13, 0)], [Q_A, Q_B]),              # 63, 64, 65
        make_info(hvc, [(16, 16, 0), (0, 4, 0), (1, 257, 1)], [Q_B, Q_A]),           # 256, empty, bw == 1 with 257
        make_info(hvc, [(4, 0, 0)], [Q_A]),                                          # a frame without a block
        make_info(hvc, [(3, 2, 0), (3, 2, 1)], [Q_WIDE, Q_A]),
    ]
    coef, pix, co, po = [], [], 0, 0
    for i in infos:
        coef.append(co)
        pix.append(po)
        co += i.coef_count
        po += (i.pixel_bytes + 255) // 256 * 256
    plan = run_builder(harness, tmp_path, infos, coef, pix)
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert [p["nblk"] for p in plan["planes"]] == [1, 63, 64, 65, 256, 257, 6, 6]    # the empty planes have no descriptor
    assert [p["bw"] for p in plan["planes"]] == [1, 9, 8, 5, 16, 1, 3, 3]
    assert plan["blocks"] == sum(p["nblk"] for p in plan["planes"])
    # units: ceil(nblk / 64) per plane, in order; every map entry names its plane
    want_map = []
    for k, p in enumerate(plan["planes"]):
        assert p["unit0"] == len(want_map)
        want_map += [k] * (-(-p["nblk"] // 64))
    assert plan["map"] == want_map and len(want_map) == 1 + 1 + 1 + 2 + 4 + 5 + 1 + 1
    # every block in exactly one (unit, lane), by the kernel's own arithmetic
    for k, p in enumerate(plan["planes"]):
        seen = np.zeros(p["nblk"], dtype=int)
        for u in [u for u, pl in enumerate(plan["map"]) if pl == k]:
            for lane in range(64):
                b = (u - p["unit0"]) * 64 + lane
                if b < p["nblk"]:
                    by = b if p["bw"] == 1 else (b * p["magic"]) >> 32
                    bx = b - by * p["bw"]
                    assert 0 <= bx < p["bw"]
                    seen[by * p["bw"] + bx] += 1
        assert (seen == 1).all(), k
    # tables: three distinct contents among the eight planes
    assert len(plan["tables"]) == 3
    tabs = [tuple(t["qt"]) for t in plan["tables"]]
    assert tabs == [tuple(Q_A), tuple(Q_B), tuple(Q_WIDE)]
    assert [p["table"] for p in plan["planes"]] == [0, 0, 1, 0, 1, 0, 2, 0]
    assert [t["wide"] for t in plan["tables"]] == [0, 0, 1]
    for t in plan["tables"]:
        qmax = max(t["qt"])
        assert t["ethr"] == min((32767 // qmax) ** 2, 0x7ffffffe)
    # bases: the frame's offset plus the plane's
    assert plan["planes"][3]["coef_base"] == coef[1] + (63 + 64) * 64 and plan["planes"][3]["pix_base"] == pix[1] + (63 + 64) * 64
    # the operand pairs of row r: natural positions (1, 7) (5, 3) (2, 6) (0, 4) of hvc_idct_spec.h, zig-zag indexed
    ZF = [0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
          10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63]
    for t in plan["tables"]:
        for r in range(8):
            for k, (lo, hi) in enumerate(((1, 7), (5, 3), (2, 6), (0, 4))):
                assert t["qpair"][4 * r + k] == t["qt"][ZF[8 * r + lo]] | (t["qt"][ZF[8 * r + hi]] << 16)


def test_a_list_of_frames_leaves_the_others_out(hvc, harness, tmp_path):
    infos = [make_info(hvc, [(2, 2, 0)], [Q_A]), make_info(hvc, [(70, 1, 0)], [Q_B]), make_info(hvc, [(3, 3, 0)], [Q_A])]
    plan = run_builder(harness, tmp_path, infos, [0, 256, 256 + 4480], [0, 256, 256 + 4608], frames=[2, 0])
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert [p["nblk"] for p in plan["planes"]] == [9, 4] and len(plan["tables"]) == 1 and plan["map"] == [0, 1]
    assert plan["planes"][0]["coef_base"] == 256 + 4480 and plan["planes"][1]["coef_base"] == 0
    none = run_builder(harness, tmp_path, infos, [0, 0, 0], [0, 0, 0], frames=[])
    assert none["status"] == 0 and none["planes"] == [] and none["map"] == [] and none["blocks"] == 0


def test_alignment_and_arguments(hvc, harness, tmp_path):
    info = make_info(hvc, [(2, 2, 0), (1, 1, 0)], [Q_A])
    assert run_builder(harness, tmp_path, [info], [0], [0])["status"] == 0
    assert run_builder(harness, tmp_path, [info], [0], [4])["status"] == -4      # a pixel plane off 8 bytes
    assert run_builder(harness, tmp_path, [info], [4], [0])["status"] == -4      # a coefficient plane off 16 bytes
    assert run_builder(harness, tmp_path, [info], [8], [8])["status"] == 0
    odd = make_info(hvc, [(2, 2, 0)], [Q_A])
    odd.layout[0].stride = 20
    assert run_builder(harness, tmp_path, [odd], [0], [0])["status"] == -4
    odd.layout[0].stride = 8
    assert run_builder(harness, tmp_path, [odd], [0], [0])["status"] == -1       # a stride below the row
    bad = make_info(hvc, [(2, 2, 1)], [Q_A])
    assert run_builder(harness, tmp_path, [bad], [0], [0])["status"] == -1       # a table the frame does not have
    # sums of coef_count and the records of hvc_jpeg_mixed_layout always satisfy the rules
    files = [golden_bytes("mini.jpg"), unusual_sampling_file(UNUSUAL_SAMPLINGS[7], 97, 51, 3)[0], golden_bytes("Mouse480.jpg")]
    lay = hvc.jpeg_mixed_layout(files, 8)
    coef = np.concatenate([[0], np.cumsum([lay.infos[f].coef_count for f in range(3)])])[:3]
    plan = run_builder(harness, tmp_path, list(lay.infos), [int(x) for x in coef], list(lay.pixel_offsets))
    assert plan["status"] == 0 and plan["check"] == "ok" and plan["blocks"] == sum(lay.infos[f].coef_count for f in range(3)) // 64


def test_seeded_random_sets_in_the_sanitizer_build(harness):
    r = subprocess.run([harness, "random", "20261018", "400"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.split()[:2] == ["ok", "400"]
