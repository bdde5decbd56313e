"""The host plan of the mixed GPU Huffman coder (csrc/hvc_huff_mixed_plan.cpp), without a GPU, through the stand-alone program
tests/host_harness/huff_mixed_plan_harness.cpp, which runs it under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only
g++ build: tests/host_harness/Makefile.huff_mixed).  Nothing loaded into Python runs under a sanitizer."""
import ctypes as C
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
E_INVALID_ARG, E_ALIGNMENT, E_TOO_LARGE = -1, -4, -7


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("huff_mixed") / "huff_mixed_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.huff_mixed", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def frame(hvc, w, h, chroma, q=75):
    info = hvc.JpegInfo()
    assert hvc.lib().hvc_jpeg_encoder_layout(w, h, chroma, q, C.byref(info)) == 0
    return info


def copy_of(hvc, info):
    return hvc.JpegInfo.from_buffer_copy(bytes(info))


def run_plan(harness, tmp_path, infos, coef_offsets, frames=None, optimised=False):
    n = len(infos)
    raw = struct.pack("<qq", n, -1 if frames is None else len(frames)) + b"".join(bytes(i) for i in infos)
    raw += struct.pack("<%dQ" % n, *coef_offsets)
    if frames is not None:
        raw += struct.pack("<%di" % len(frames), *frames)
    p = tmp_path / "set.bin"
    p.write_bytes(raw)
    r = subprocess.run([harness, "dump", str(p), "1" if optimised else "0"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(files=[], planes=[], map=[], codes=[], file_of=[])
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "status":
            out["status"] = int(w[1])
        elif w[0] in ("sizes", "totals", "codes", "file_of", "map"):
            out[w[0]] = list(map(int, w[1:]))
        elif w[0] == "file":
            out["files"].append(dict(zip(("mbs_wide", "mbs_high", "blocks_per_mcu", "blocks", "lens_base", "bitbuf_base", "bitbuf_words"),
                                         map(int, w[2:]))))
        elif w[0] == "plane":
            out["planes"].append(dict(zip(("coef_base", "bw", "nblk", "h", "v", "mcu_base", "table", "unit0", "file"), map(int, w[2:]))))
    return out


def offsets_of(infos):
    out, at = [], 0
    for i in infos:
        out.append(at)
        at += (i.coef_count + 7) // 8 * 8
    return out


def check_plan(plan, infos, coef, taken):
    """every descriptor, map entry and base of `plan` again, from the infos of the frames `taken` (in plan order)"""
    assert plan["status"] == 0 and plan["file_of"] == taken
    assert plan["sizes"][0] == len(taken) and plan["sizes"][3] == 3 * len(taken)
    lens = words = units = elems = 0
    want_map = []
    for k, f in enumerate(taken):
        info, F = infos[f], plan["files"][k]
        c0 = info.comp[0]
        mw, mh = c0.decoded_width // (8 * c0.hscale), c0.decoded_height // (8 * c0.vscale)
        per = sum(info.comp[i].hscale * info.comp[i].vscale for i in range(3))
        assert (F["mbs_wide"], F["mbs_high"], F["blocks_per_mcu"], F["blocks"]) == (mw, mh, per, mw * mh * per)
        # the bit buffer: 216 bytes per coded block (+ 8), in whole 64-byte pieces, each file on a piece of its own
        assert F["bitbuf_words"] == (((F["blocks"] * 216 + 3) // 4 + 2) + 15) // 16 * 16
        assert (F["lens_base"], F["bitbuf_base"]) == (lens, words) and words % 16 == 0
        lens += F["blocks"]
        words += F["bitbuf_words"]
        elems += info.coef_count
        base = 0
        for i in range(3):
            P, L, K = plan["planes"][3 * k + i], info.layout[i], info.comp[i]
            assert (P["bw"], P["nblk"], P["h"], P["v"]) == (L.blocks_w, L.blocks_w * L.blocks_h, K.hscale, K.vscale)
            assert (P["mcu_base"], P["table"], P["file"]) == (base, 1 if K.dc_table else 0, k)
            assert P["coef_base"] == coef[f] + L.coef_offset and P["unit0"] == units
            n_units = -(-P["nblk"] // 64)
            want_map += [3 * k + i] * n_units
            units += n_units
            base += K.hscale * K.vscale
    assert plan["map"] == want_map
    assert plan["totals"] == [lens, words, words // 16, elems]


def test_descriptors_maps_and_bases(hvc, harness, tmp_path):
    """planes of 1, 63, 64, 65, 256 and 257 blocks (the last with bw == 1), and the subsampled geometries whose planes are
    larger than the MCU grid"""
    infos = [frame(hvc, 8, 8, 444), frame(hvc, 72, 56, 444), frame(hvc, 64, 64, 444), frame(hvc, 40, 104, 444),
             frame(hvc, 128, 128, 444), frame(hvc, 8, 2056, 444), frame(hvc, 24, 24, 420), frame(hvc, 40, 24, 422),
             frame(hvc, 2, 2, 420), frame(hvc, 520, 264, 422)]
    coef = offsets_of(infos)
    plan = run_plan(harness, tmp_path, infos, coef)
    assert [p["nblk"] for p in plan["planes"][:18:3]] == [1, 63, 64, 65, 256, 257] and plan["planes"][15]["bw"] == 1
    assert plan["codes"] == [0] * len(infos)
    check_plan(plan, infos, coef, list(range(len(infos))))
    assert plan["files"][9]["blocks"] > 4096   # more lengths than a round of the per-file scan takes
    # a list that leaves frames out, in an order of its own
    part = run_plan(harness, tmp_path, infos, coef, frames=[5, 0, 6])
    check_plan(part, infos, coef, [5, 0, 6])
    none = run_plan(harness, tmp_path, infos, coef, frames=[])
    assert none["status"] == 0 and none["sizes"] == [0, 0, 0, 0, 0] and none["totals"] == [0, 0, 0, 0]
    empty = run_plan(harness, tmp_path, [], [])
    assert empty["status"] == 0 and empty["sizes"] == [0, 0, 0, 0, 0]
    # optimised tables: the same plan for frames with two table sets
    check_plan(run_plan(harness, tmp_path, infos, coef, optimised=True), infos, coef, list(range(len(infos))))


def test_every_refusal_has_its_code_and_leaves_no_half_made_plan(hvc, harness, tmp_path):
    good_a, good_b = frame(hvc, 24, 24, 420), frame(hvc, 72, 64, 444)
    refused = frame(hvc, 33, 16, 420)            # hvc_jpeg_encoder_check's refusal: the MCU grid leaves the chroma planes
    assert hvc.lib().hvc_jpeg_encoder_check(C.byref(refused)) == E_INVALID_ARG
    mono = copy_of(hvc, good_a)
    mono.n_comp = 1
    no_mcu = copy_of(hvc, good_a)                # no coded block: a luma plane narrower than one MCU
    no_mcu.comp[0].decoded_width = 8
    huge = frame(hvc, 8000, 8000, 444)           # 3 000 000 blocks x 64 x 27 bits: beyond 32-bit bit offsets
    one_set = copy_of(hvc, good_b)               # all components on table set 0: no symbol to fit set 1 to
    for i in range(3):
        one_set.comp[i].dc_table = one_set.comp[i].ac_table = 0
    off_16 = copy_of(hvc, good_b)                # a coefficient plane off 16 bytes
    off_16.layout[1].coef_offset += 4
    infos = [good_a, refused, mono, no_mcu, good_b, huge, one_set, off_16, good_a]
    coef = offsets_of(infos)
    only = run_plan(harness, tmp_path, infos, coef, frames=[0, 4, 8])
    for optimised in (False, True):
        plan = run_plan(harness, tmp_path, infos, coef, optimised=optimised)
        want = [0, E_INVALID_ARG, E_INVALID_ARG, E_INVALID_ARG, 0, E_TOO_LARGE, E_INVALID_ARG if optimised else 0, E_ALIGNMENT, 0]
        assert plan["status"] == 0 and plan["codes"] == want
        taken = [f for f, c in enumerate(want) if c == 0]
        check_plan(plan, infos, coef, taken)     # the refused frames took no unit, no length, no word
        if optimised:
            assert plan["files"] == only["files"] and plan["map"] == only["map"] and plan["totals"] == only["totals"]
    # a record that is not on 16 bytes
    assert run_plan(harness, tmp_path, [good_a, good_b], [0, coef[1] + 4])["codes"] == [0, E_ALIGNMENT]
    # what concerns the call: nothing is left
    bad = run_plan(harness, tmp_path, infos, coef, frames=[0, -1])
    assert bad["status"] == E_INVALID_ARG and bad["sizes"] == [0, 0, 0, 0, 0] and bad["totals"] == [0, 0, 0, 0]


def hand_back(harness, cap, offsets, status):
    args = [str(cap), str(len(status))] + [str(o) for o in offsets] + [str(s) for s in status]
    r = subprocess.run([harness, "handback"] + args, capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0].split()[0] == "complete" and lines[1].split()[0] == "back"
    return list(map(int, lines[0].split()[1:])), list(map(int, lines[1].split()[1:]))


def test_hand_back_decision(harness):
    off = [0, 100, 250, 250, 400]
    assert hand_back(harness, 400, off, [0, 0, 0, 0]) == ([0, 1, 2, 3], [])           # the capacity hit exactly
    assert hand_back(harness, 399, off, [0, 0, 0, 0]) == ([0, 1, 2], [3])             # one byte past
    assert hand_back(harness, 249, off, [0, 0, 0, 0]) == ([0], [1, 2, 3])             # every file from the first that ends past it
    assert hand_back(harness, 400, off, [0, 0, 1, 0]) == ([0, 1, 3], [2])             # a flagged file in the middle (it holds no byte)
    assert hand_back(harness, 120, off, [1, 0, 0, 0]) == ([], [0, 1, 2, 3])
    assert hand_back(harness, 0, [0], []) == ([], [])
