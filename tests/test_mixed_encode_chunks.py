"""The chunk cut of the two mixed ENCODE file pipelines (csrc/hvc_mixed_encode_chunks.cpp) and pad_frame, without a GPU: the
stand-alone program tests/host_harness/mixed_encode_chunks_harness.cpp runs them under AddressSanitizer and
UndefinedBehaviorSanitizer (a CPU-only g++ build: tests/host_harness/Makefile.mixed_encode_chunks) and prints the plan; the plan
it is compared with is computed here.  The infos are hvc_jpeg_encoder_mixed_layout's.  Nothing loaded into Python runs under a
sanitizer.

The frames: 8x8 4:4:4, 16x16 4:2:0, 16x8 4:2:2, 24x17 4:2:0, 9x9 4:4:4 -- and 24x18 4:2:0, because hvc_jpeg_encoder_check refuses
24x17 4:2:0 (an odd height under 4:2:0 whose luma MCU rows outnumber the chroma's): in the chunk cases it is the frame that
arrives with the layout call's status, or is refused by the check; 24x18 is the frame with padding rows that takes part, so
that five frames do."""
import ctypes as C
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}

SET = [(8, 8, 444, 75), (16, 16, 420, 75), (16, 8, 422, 75), (24, 17, 420, 75), (9, 9, 444, 75), (24, 18, 420, 75)]
GOOD = [0, 1, 2, 4, 5]
PIXEL_BYTES = {0: 192, 1: 384, 2: 512, 4: 768, 5: 1536}     # the padded planes: 3 * 8 * 8, 256 + 2 * 64, 256 + 2 * 128, ...
INVALID_ARG, RANGE = -1, -5


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixed_encode_chunks") / "mixed_encode_chunks_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.mixed_encode_chunks", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def lay(hvc):
    lay = hvc.jpeg_encoder_mixed_layout(SET)
    assert [lay.status[f] for f in range(len(SET))] == [0, 0, 0, INVALID_ARG, 0, 0]
    assert {f: lay.infos[f].pixel_bytes for f in GOOD} == PIXEL_BYTES
    return lay


def copy_of(info):
    return type(info).from_buffer_copy(bytes(info))


def up(v, a):
    return (v + a - 1) // a * a


def run_plan(harness, tmp_path, infos, status, chunk_bytes=0, cap=0, rgb=None, strides=None, no_frame=(), no_jpeg=()):
    """rgb: None or the layout (0 interleaved, 1 planar) -> what the harness printed, as a dict"""
    n = len(infos)
    raw = struct.pack("<6q", n, chunk_bytes, cap, 0 if rgb is None else 1, rgb or 0, 0 if strides is None else 1)
    raw += b"".join(bytes(i) for i in infos) + struct.pack("<%di" % n, *status)
    raw += bytes(0 if f in no_frame else 1 for f in range(n)) + bytes(0 if f in no_jpeg else 1 for f in range(n))
    if strides is not None:
        raw += struct.pack("<%dQ" % n, *strides)
    p = tmp_path / "set.bin"
    p.write_bytes(raw)
    r = subprocess.run([harness, "plan", str(p)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(chunks=[])
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "status":
            out["status"] = int(w[1])
        elif w[0] == "chunk":
            out["chunks"].append(dict(zip(("first", "count", "pix_bytes", "coef_elems", "rgb_bytes"), map(int, w[2:]))))
        elif w[0] == "wants":
            out["wants"] = dict(zip(("in_bytes", "out_bytes", "rgb_bytes", "largest", "coef_total"), map(int, w[1:])))
        else:
            out[w[0]] = list(map(int, w[1:]))
    return out


def expected_plan(infos, status, chunk_bytes=0, cap=0, rgb=None, refused=None):
    """The plan as the issue words it.  refused: frame -> the code it is refused with (its own refusal is the test's to name)."""
    n = len(infos)
    chunk_bytes = chunk_bytes or 64 << 20
    statuses = list(status)
    take, chunk_of, chunks = [], [-1] * n, []
    pix_rel, coef_rel, rgb_rel = [0] * n, [0] * n, ([0] * n if rgb is not None else [])
    for f in range(n):
        if statuses[f] != 0:
            continue
        if refused and f in refused:
            statuses[f] = refused[f]
            continue
        pb = up(infos[f].pixel_bytes, 64)
        if not chunks or (chunks[-1]["count"] > 0 and (chunks[-1]["pix_bytes"] + pb > chunk_bytes or (cap and chunks[-1]["count"] >= cap))):
            chunks.append(dict(first=len(take), count=0, pix_bytes=0, coef_elems=0, rgb_bytes=0))
        k = chunks[-1]
        pix_rel[f], coef_rel[f], chunk_of[f] = k["pix_bytes"], k["coef_elems"], len(chunks) - 1
        k["pix_bytes"] += pb
        k["coef_elems"] += up(infos[f].coef_count, 32)
        if rgb is not None:
            rgb_rel[f] = k["rgb_bytes"]
            k["rgb_bytes"] += up(3 * infos[f].width * infos[f].height, 64)      # either layout: three bytes a pixel, rows tight
        k["count"] += 1
        take.append(f)
    wants = dict(in_bytes=max([max(k["pix_bytes"], k["rgb_bytes"]) for k in chunks], default=0),
                 out_bytes=max([2 * k["coef_elems"] for k in chunks], default=0),
                 rgb_bytes=max([k["rgb_bytes"] for k in chunks], default=0),
                 largest=max([k["count"] for k in chunks], default=0), coef_total=sum(2 * k["coef_elems"] for k in chunks))
    return dict(status=0, statuses=statuses, take=take, chunk_of=chunk_of, chunks=chunks, pix_rel=pix_rel, coef_rel=coef_rel,
                rgb_rel=rgb_rel, wants=wants)


def check_alignment(plan, infos):
    """offsets on 64 bytes / 32 elements, each the running sum of the rounded records of the frames before it in its chunk"""
    for k in plan["chunks"]:
        pix = coef = rgb = 0
        for f in plan["take"][k["first"]:k["first"] + k["count"]]:
            assert (plan["pix_rel"][f], plan["coef_rel"][f]) == (pix, coef) and pix % 64 == 0 and coef % 32 == 0
            pix += up(infos[f].pixel_bytes, 64)
            coef += up(infos[f].coef_count, 32)
            if plan["rgb_rel"]:
                assert plan["rgb_rel"][f] == rgb and rgb % 64 == 0
                rgb += up(3 * infos[f].width * infos[f].height, 64)
        assert (k["pix_bytes"], k["coef_elems"]) == (pix, coef) and k["rgb_bytes"] == rgb


@pytest.mark.parametrize("chunk_bytes,counts", [(0, [5]), (64, [1, 1, 1, 1, 1]), (600, [2, 1, 1, 1]), (1300, [3, 1, 1]), (1536, [3, 1, 1]),
                                                (1 << 20, [5])])
def test_chunk_counts(harness, tmp_path, lay, chunk_bytes, counts):
    """0 = 64 MiB: one chunk; 64: a frame per chunk; between two record sizes: several; a frame above chunk_bytes sits alone
    (600: 768 and 1536 do; 1300 and 1536 = exactly the record: the last one does)"""
    infos, status = list(lay.infos), list(lay.status)
    got = run_plan(harness, tmp_path, infos, status, chunk_bytes)
    assert got == expected_plan(infos, status, chunk_bytes)
    assert [k["count"] for k in got["chunks"]] == counts and got["take"] == GOOD
    assert got["statuses"] == status and got["chunk_of"][3] == -1               # the entry status stays, the frame is skipped
    check_alignment(got, infos)
    for k in got["chunks"]:
        assert k["count"] == 1 or k["pix_bytes"] <= (chunk_bytes or 64 << 20)


def test_file_cap(harness, tmp_path, lay):
    infos, status = list(lay.infos), list(lay.status)
    capped = run_plan(harness, tmp_path, infos, status, 0, cap=2)
    assert capped == expected_plan(infos, status, 0, cap=2) and [k["count"] for k in capped["chunks"]] == [2, 2, 1]
    assert capped["wants"]["largest"] == 2
    check_alignment(capped, infos)
    assert [k["count"] for k in run_plan(harness, tmp_path, infos, status, 1300, cap=0)["chunks"]] == [3, 1, 1]     # no cap
    both = run_plan(harness, tmp_path, infos, status, 1300, cap=4)              # whichever closes first: here the bytes
    assert both == expected_plan(infos, status, 1300, cap=4) and [k["count"] for k in both["chunks"]] == [3, 1, 1]
    both = run_plan(harness, tmp_path, infos, status, 1300, cap=2)              # ... here the cap (the bytes would take a third)
    assert both == expected_plan(infos, status, 1300, cap=2) and [k["count"] for k in both["chunks"]] == [2, 2, 1]
    assert run_plan(harness, tmp_path, infos, status, 0, cap=1) == run_plan(harness, tmp_path, infos, status, 64)


@pytest.mark.parametrize("chunk_bytes,cap,counts", [(0, 1, [1, 1, 1, 1, 1]), (0, 3, [3, 2]), (0, 5, [5]), (0, 6, [5]), (0, 4, [4, 1]),
                                                    (600, 3, [2, 1, 1, 1]), (1300, 3, [3, 1, 1]), (1 << 20, 3, [3, 2])])
def test_file_cap_values(harness, tmp_path, lay, chunk_bytes, cap, counts):
    """max_files_per_chunk as hvc_jpeg_encode_batch_mixed_gpu sets it (there: HVC_HUFF_MIXED_MAX_FILES, which
    tests/test_gpu_mixed_counts.py reaches with 65537 frames): 1, 3, exactly the files that take part (5) and the set's size (6),
    one below; and with a byte limit that closes the chunk first (600: after two files) or with the same file (1300: the
    third).  The rule restated (csrc/hvc_mixed_encode_chunks.h): a chunk that holds a file closes when the next record would
    take it past chunk_bytes or when it holds `cap` files."""
    infos, status = list(lay.infos), list(lay.status)
    got = run_plan(harness, tmp_path, infos, status, chunk_bytes, cap=cap)
    assert got == expected_plan(infos, status, chunk_bytes, cap=cap)
    assert [k["count"] for k in got["chunks"]] == counts and got["take"] == GOOD
    assert got["wants"]["largest"] == max(counts) <= cap
    check_alignment(got, infos)
    limit, first = chunk_bytes or 64 << 20, 0                                  # the rule once more, chunk by chunk
    for j, k in enumerate(got["chunks"]):
        assert 1 <= k["count"] <= cap and (k["count"] == 1 or k["pix_bytes"] <= limit)
        if j + 1 < len(got["chunks"]):                                         # why it closed: full, or the next record did not fit
            nxt = up(infos[GOOD[first + k["count"]]].pixel_bytes, 64)
            assert k["count"] == cap or k["pix_bytes"] + nxt > limit
        first += k["count"]
    assert first == len(GOOD)


@pytest.mark.parametrize("layout", [0, 1])
def test_rgb_records_and_ring_wants(harness, tmp_path, lay, layout):
    """the tight images beside the planes, on 64 bytes; in_bytes is the larger of the two per chunk (the 4:2:0 frames' images are
    larger than their planes only before padding: 9x9 4:4:4 is 243 bytes of image and 768 of planes)"""
    infos, status = list(lay.infos), list(lay.status)
    for chunk_bytes in (0, 600):
        got = run_plan(harness, tmp_path, infos, status, chunk_bytes, rgb=layout)
        assert got == expected_plan(infos, status, chunk_bytes, rgb=layout)
        check_alignment(got, infos)
        w = got["wants"]
        assert w["in_bytes"] == max(max(k["pix_bytes"], k["rgb_bytes"]) for k in got["chunks"])
        assert w["rgb_bytes"] == max(k["rgb_bytes"] for k in got["chunks"]) > 0
        assert w["out_bytes"] == max(2 * k["coef_elems"] for k in got["chunks"])
    # an image larger than its planes: 16x16 4:2:0 is 768 bytes of image, 384 of planes
    one = run_plan(harness, tmp_path, [lay.infos[1]], [0], 0, rgb=layout)
    assert one["chunks"][0]["rgb_bytes"] == 768 and one["chunks"][0]["pix_bytes"] == 384 and one["wants"]["in_bytes"] == 768
    plain = run_plan(harness, tmp_path, infos, status, 0)
    assert plain["rgb_rel"] == [] and plain["wants"]["rgb_bytes"] == 0 and plain["wants"]["in_bytes"] == plain["chunks"][0]["pix_bytes"]


def test_entry_status(harness, tmp_path, lay):
    infos, status = list(lay.infos), list(lay.status)
    status[1] = -8                                                             # not HVC_OK on entry: skipped, and it keeps the code
    got = run_plan(harness, tmp_path, infos, status, 600)
    assert got == expected_plan(infos, status, 600)
    assert got["statuses"][1] == -8 and got["statuses"][3] == INVALID_ARG and got["take"] == [0, 2, 4, 5]


def refusals(hvc, lay):
    """name -> (info, rgb layout or None, row stride or None, code): each a frame of its own that is refused"""
    def mutated(f, change):
        i = copy_of(lay.infos[f])
        change(i)
        return i

    def two_components(i):
        i.n_comp = 2

    def zero_quantiser(i):
        i.qtabs[1][9] = 0

    def plane_beside_its_blocks(i):
        i.comp[1].decoded_width += 8

    def laid_out(w, h, chroma):
        one = hvc.jpeg_encoder_mixed_layout([(w, h, chroma, 75)])
        assert one.status[0] == 0                                              # a frame the planar input takes
        return copy_of(one.infos[0])

    return {"n_comp": (mutated(1, two_components), None, None, INVALID_ARG),
            "zero_quantiser": (mutated(1, zero_quantiser), None, None, RANGE),
            "decoded_width": (mutated(2, plane_beside_its_blocks), None, None, INVALID_ARG),
            "rgb_odd_width_420": (laid_out(15, 8, 420), 0, None, INVALID_ARG),
            "rgb_odd_width_422": (laid_out(15, 8, 422), 1, None, INVALID_ARG),
            "rgb_odd_height_420": (laid_out(16, 15, 420), 0, None, INVALID_ARG),
            "rgb_short_stride": (copy_of(lay.infos[0]), 0, 3 * 8 - 1, INVALID_ARG)}


@pytest.mark.parametrize("name", ["n_comp", "zero_quantiser", "decoded_width", "encoder_check", "rgb_odd_width_420", "rgb_odd_width_422",
                                  "rgb_odd_height_420", "rgb_short_stride"])
def test_refused_frames(hvc, harness, tmp_path, lay, name):
    """the bad frame in the middle gets its code, is not in `take`, and its neighbours lie where they lie without it"""
    if name == "encoder_check":     # 24x17 4:2:0 laid out by hvc_jpeg_encoder_layout, arriving as HVC_OK: the check's refusal
        bad = hvc.JpegInfo()
        assert hvc.lib().hvc_jpeg_encoder_layout(24, 17, 420, 75, C.byref(bad)) == 0
        assert hvc.lib().hvc_jpeg_encoder_check(C.byref(bad)) == INVALID_ARG
        rgb, stride, code = None, None, INVALID_ARG
    else:
        bad, rgb, stride, code = refusals(hvc, lay)[name]
    good = [lay.infos[f] for f in GOOD]
    infos = good[:2] + [bad] + good[2:]
    strides = None if stride is None else [0, 0, stride, 0, 0, 0]
    for chunk_bytes in (0, 600):
        got = run_plan(harness, tmp_path, infos, [0] * 6, chunk_bytes, rgb=rgb, strides=strides)
        assert got == expected_plan(infos, [0] * 6, chunk_bytes, rgb=rgb, refused={2: code})
        assert got["statuses"] == [0, 0, code, 0, 0, 0] and got["take"] == [0, 1, 3, 4, 5] and got["chunk_of"][2] == -1
        without = run_plan(harness, tmp_path, good, [0] * 5, chunk_bytes, rgb=rgb)
        assert without["statuses"] == [0] * 5
        for key in ("pix_rel", "coef_rel", "rgb_rel", "chunk_of"):
            assert [v for f, v in enumerate(got[key]) if f != 2] == without[key], key
        assert got["chunks"] == without["chunks"] and got["wants"] == without["wants"]
    if rgb is not None:             # the same frame is taken as a planar one, and with a row stride that holds the row
        assert run_plan(harness, tmp_path, infos, [0] * 6, 0)["statuses"] == [0] * 6
    if stride is not None:
        assert run_plan(harness, tmp_path, infos, [0] * 6, 0, rgb=rgb, strides=[0, 0, stride + 1, 0, 0, 0])["statuses"] == [0] * 6


def test_null_pointers(harness, tmp_path, lay):
    bad = copy_of(lay.infos[0])
    bad.n_comp = 2
    infos = [bad, lay.infos[1], lay.infos[2], lay.infos[4]]
    for kind in ("no_frame", "no_jpeg"):
        got = run_plan(harness, tmp_path, infos, [0] * 4, 0, **{kind: (2,)})
        assert got["status"] == INVALID_ARG and got["statuses"] == [INVALID_ARG, 0, 0, 0]    # frame 0's refusal is still there
        # ... of a frame that takes part: one that arrives refused needs neither
        assert run_plan(harness, tmp_path, infos, [0, 0, -8, 0], 0, **{kind: (2,)})["status"] == 0
    # records that span more than the info says: the call's error, too
    short = copy_of(lay.infos[1])
    short.pixel_bytes -= 64
    assert run_plan(harness, tmp_path, [lay.infos[0], short], [0, 0], 0)["status"] == INVALID_ARG


def test_empty_sets(harness, tmp_path, lay):
    empty = dict(in_bytes=0, out_bytes=0, rgb_bytes=0, largest=0, coef_total=0)
    none = run_plan(harness, tmp_path, [], [], 0)
    assert none["status"] == 0 and none["take"] == [] and none["chunks"] == [] and none["wants"] == empty
    bad = copy_of(lay.infos[0])
    bad.n_comp = 2
    got = run_plan(harness, tmp_path, [bad, lay.infos[3], lay.infos[1]], [0, lay.status[3], -8], 64)
    assert got["status"] == 0 and got["take"] == [] and got["chunks"] == [] and got["wants"] == empty
    assert got["statuses"] == [INVALID_ARG, INVALID_ARG, -8] and got["chunk_of"] == [-1, -1, -1]


def test_the_uniform_pipelines_plane_sizes_are_the_infos(harness):
    """hvc_jpeg_encode_batch pads with pad_frame too: hvc_jpeg_encoder_layout's actual plane sizes are what it used to derive from
    width, height and chroma -- every size up to 70 x 40, odd and even, under 4:2:0, 4:2:2 and 4:4:4"""
    r = subprocess.run([harness, "rule", "70", "40"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    laid_out, checked, differ = map(int, r.stdout.splitlines()[-1].split()[1:])
    assert laid_out == 3 * 70 * 40 and checked > laid_out // 2 and differ == 0, r.stdout[-2000:]


@pytest.mark.parametrize("w,h,chroma", [(24, 17, 420), (9, 9, 444), (16, 8, 422)])
def test_pad_frame(harness, w, h, chroma):
    """own samples copied, right and bottom padding zero, nothing else of the 0xA5-filled record and its guard touched"""
    r = subprocess.run([harness, "pad", str(w), str(h), str(chroma)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[0].split()[:2] == ["layout", "0"]
    cw, ch = (w if chroma == 444 else w // 2), (h // 2 if chroma == 420 else h)
    pixel_bytes = int(lines[4].split()[1])
    want = bytearray(b"\xa5" * (pixel_bytes + 64))
    at = 0
    for i, (sw, sh) in enumerate(((w, h), (cw, ch), (cw, ch))):
        f = lines[1 + i].split()
        assert (int(f[3]), int(f[4])) == (int(f[6]), int(f[7])) == (sw, sh)
        pw, ph, off, stride = int(f[9]), int(f[10]), int(f[12]), int(f[14])
        assert pw >= sw and ph >= sh and pw % 8 == 0 and ph % 8 == 0
        for row in range(ph):
            own = bytes((at + row * sw + x) % 251 + 1 for x in range(sw)) if row < sh else b""
            want[off + row * stride:off + row * stride + pw] = own + bytes(pw - len(own))
        at += sw * sh
    got = bytes.fromhex(lines[5].split()[1])
    assert got == bytes(want)
    assert got[pixel_bytes:] == b"\xa5" * 64
    if (w, h, chroma) == (24, 17, 420):
        assert got[17 * 32:32 * 32] == bytes(15 * 32) and got[16 * 32 + 24:17 * 32] == bytes(8)   # padding rows; right of the last own row
