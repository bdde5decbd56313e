"""The chunk cut of the mixed DECODE file pipeline and the copies that take a chunk's output back to host memory
(csrc/hvc_mixed_decode_chunks.cpp), without a GPU: the stand-alone program tests/host_harness/mixed_decode_chunks_harness.cpp
runs them under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only g++ build:
tests/host_harness/Makefile.mixed_decode_chunks) and prints the plan and the runs; what they are compared with is computed
here, from the rules as csrc/hvc_mixed_decode_chunks.h words them.  The infos are hvc_jpeg_encoder_mixed_layout's (a decoder's
info of the file such a frame becomes has the same layout).  Nothing loaded into Python runs under a sanitizer.

The files: 8x8 4:4:4, 16x16 4:2:0, 16x8 4:2:2, 24x18 4:2:0, 9x9 4:4:4 -- coefficient records of 384, 768, 1024, 3072 and 1536
bytes, planes of 192, 384, 512, 1536 and 768 -- and a four-component info made by hand, which no RGB form takes."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}

SET = [(8, 8, 444, 75), (16, 16, 420, 75), (16, 8, 422, 75), (24, 18, 420, 75), (9, 9, 444, 75)]
COEF_BYTES = [384, 768, 1024, 3072, 1536]
PIXEL_BYTES = [192, 384, 512, 1536, 768]
OK, INVALID_ARG, ALIGNMENT, TOO_LARGE, BAD_JPEG = 0, -1, -4, -7, -8
HOST, DEVICE = 0, 1
BOX, BILINEAR, BICUBIC = 0, 1, 2
OUT_SIZES = [(5, 7), (8, 8), (20, 3), (12, 12), (9, 4)]       # what the resized form takes the five images to
FORMS = ["planes", "rgb", "rgb_planar", "scale2", "scale4", "scale8", "resized"]


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mixed_decode_chunks") / "mixed_decode_chunks_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.mixed_decode_chunks", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert not r.stdout.strip() and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]      # no warning either
    return exe


@pytest.fixture(scope="module")
def infos(hvc):
    lay = hvc.jpeg_encoder_mixed_layout(SET)
    assert [lay.status[f] for f in range(5)] == [0] * 5
    assert [2 * lay.infos[f].coef_count for f in range(5)] == COEF_BYTES and [lay.infos[f].pixel_bytes for f in range(5)] == PIXEL_BYTES
    return [copy_of(lay.infos[f]) for f in range(5)]


def copy_of(info):
    return type(info).from_buffer_copy(bytes(info))


def four_components(info):
    """the info of a four-component file, made by hand: what the planes form takes and no RGB form does"""
    i = copy_of(info)
    i.n_comp = 4
    i.comp[3] = i.comp[2]
    i.layout[3] = i.layout[2]
    return i


def up(v, a):
    return (v + a - 1) // a * a


class Form:
    """MixedForm: rgb = None or the layout (0 interleaved, 1 planar); sizes = None or the (out_w, out_h) per file"""

    def __init__(self, rgb=None, scale=1, strides=None, sizes=None, filter=BILINEAR, heights=True):
        self.rgb, self.scale, self.strides, self.sizes, self.filter, self.heights = rgb, scale, strides, sizes, filter, heights

    @property
    def resized(self):
        return self.rgb is not None and self.sizes is not None

    def but(self, **kw):
        f = Form(self.rgb, self.scale, self.strides, self.sizes, self.filter, self.heights)
        for k, v in kw.items():
            setattr(f, k, v)
        return f


def form_of(name, n=5):
    return {"planes": Form(), "rgb": Form(rgb=0), "rgb_planar": Form(rgb=1), "scale2": Form(scale=2), "scale4": Form(scale=4),
            "scale8": Form(scale=8), "resized": Form(rgb=0, sizes=(OUT_SIZES * 2)[:n])}[name]


# ---------------------------------------------------------------------------------------------------------------------------
# the rules of csrc/hvc_mixed_decode_chunks.h, restated

def output_of(info, form):
    """-> (width, height, pixel_bytes) of what describes the file's output: its info, or hvc_jpeg_scaled_info of it"""
    n = 8 // form.scale
    planes = sum(info.layout[i].blocks_w * n * info.layout[i].blocks_h * n for i in range(min(info.n_comp, 4))
                 if info.layout[i].blocks_w > 0 and info.layout[i].blocks_h > 0)
    return -(-info.width * n // 8), -(-info.height * n // 8), planes if form.scale != 1 else info.pixel_bytes


def known_sampling(info):
    if info.n_comp == 1:
        return True
    if info.n_comp != 3:
        return False
    y, cb, cr = [(info.comp[i].hscale, info.comp[i].vscale) for i in range(3)]
    return cb == cr and cb[0] >= 1 and cb[1] >= 1 and y in ((cb[0], cb[1]), (2 * cb[0], 2 * cb[1]), (2 * cb[0], cb[1]))


def row_bytes(layout, w):
    return w if layout == 1 else 3 * w


def rows_of(layout, h):
    return 3 * h if layout == 1 else h


def span(layout, w, h, stride):
    return 0 if w < 1 or h < 1 else (rows_of(layout, h) - 1) * stride + row_bytes(layout, w)


def record_bytes(info, form, f):
    """out_bytes of a file that is not refused"""
    w, h, planes = output_of(info, form)
    if form.rgb is None:
        return planes
    if form.resized:
        w, h = form.sizes[f]
    stride = form.strides[f] if form.strides else 0
    return span(form.rgb, w, h, stride or row_bytes(form.rgb, w))


def expected_plan(infos, status, offsets, cap, form, chunk_bytes=0, where=HOST, have_pixels=True, no_jpeg=(), resize_status=None):
    """resize_status: file -> what resize_image_status answers for it, where that is not HVC_OK (the test's to name)"""
    n = len(infos)
    statuses = list(status)

    def call(code):
        return dict(status=code, statuses=statuses)

    if form.scale not in (1, 2, 4, 8):
        return call(INVALID_ARG)
    if n and form.resized and (not form.heights or form.filter not in (BOX, BILINEAR, BICUBIC)):
        return call(INVALID_ARG)
    limit = chunk_bytes or 64 << 20
    rgb, resized = form.rgb is not None, form.resized
    take, chunk_of, chunks = [], [-1] * n, []
    coef_rel, pix_rel, out_bytes = [0] * n, [0] * n, [0] * n
    plane_rel, rowb, rows = ([0] * n, [0] * n, [0] * n) if rgb else ([], [], [])
    rgb_rel, rimg = ([0] * n, [[0] * 8 for _ in range(n)]) if resized else ([], [])
    scaled = [[0, 0, 0] for _ in range(n)] if form.scale != 1 else []
    need = False
    for f in range(n):
        if statuses[f] != OK:
            continue
        i = infos[f]
        if f in no_jpeg or not 0 <= i.n_comp <= 4:
            return call(INVALID_ARG)
        w, h, planes = output_of(i, form)
        if scaled:
            scaled[f] = [w, h, planes]
        stride = form.strides[f] if form.strides else 0
        if rgb:
            if not known_sampling(i):
                statuses[f] = INVALID_ARG
                continue
            if w < 0 or h < 0:
                return call(INVALID_ARG)
            ow, oh = form.sizes[f] if resized else (w, h)
            if resized:
                rr = (resize_status or {}).get(f, OK)
                if rr or (stride and stride < row_bytes(form.rgb, ow)):
                    statuses[f] = rr or INVALID_ARG
                    continue
            tight = row_bytes(form.rgb, ow)
            if stride and stride < tight:
                return call(INVALID_ARG)
            rowb[f], rows[f] = tight, rows_of(form.rgb, oh)
            ob = span(form.rgb, ow, oh, stride or tight)
        else:
            ob = planes
            if form.scale == 1 and ob and offsets[f] % 8:
                return call(ALIGNMENT)
        out_bytes[f] = ob
        if ob:
            if offsets[f] > cap or offsets[f] + ob > cap:
                return call(INVALID_ARG)
            need = True
        cb = 2 * i.coef_count
        if not chunks or (chunks[-1]["count"] > 0 and chunks[-1]["coef_bytes"] + cb > limit):
            chunks.append(dict(first=len(take), count=0, coef_bytes=0, pix_lo=0, pix_hi=0, plane_bytes=0, rgb_bytes=0, mid_bytes=0, los=[]))
        k = chunks[-1]
        coef_rel[f], chunk_of[f] = k["coef_bytes"] // 2, len(chunks) - 1
        if ob:
            k["los"].append(offsets[f] // 8 * 8)
            k["pix_lo"], k["pix_hi"] = min(k["los"]), max(k["pix_hi"], offsets[f] + ob)
        if rgb:
            plane_rel[f] = k["plane_bytes"]
            k["plane_bytes"] += up(planes, 64)
        if resized:
            rgb_rel[f] = k["rgb_bytes"]
            rimg[f] = [w, h, ow, oh, k["rgb_bytes"], 0, offsets[f], stride]
            k["rgb_bytes"] += up(span(form.rgb, w, h, row_bytes(form.rgb, w)), 64)
            k["mid_bytes"] += 64 + up(row_bytes(form.rgb, ow), 4) * h * (3 if form.rgb == 1 else 1)
        k["coef_bytes"] += cb
        k["count"] += 1
        take.append(f)
    if need and not have_pixels:
        return call(INVALID_ARG)
    for k in chunks:
        del k["los"]
    if where == HOST:
        for f in take:
            pix_rel[f] = offsets[f] - chunks[chunk_of[f]]["pix_lo"] if out_bytes[f] else 0
            if resized:
                rimg[f][6] = pix_rel[f]
    wants = dict(coef=max([k["coef_bytes"] for k in chunks], default=0),
                 out=max([k["pix_hi"] - k["pix_lo"] for k in chunks], default=0) if where == HOST else 0,
                 plane=max([k["plane_bytes"] for k in chunks], default=0), rgb=max([k["rgb_bytes"] for k in chunks], default=0),
                 mid=max([k["mid_bytes"] for k in chunks], default=0), largest=max([k["count"] for k in chunks], default=0))
    return dict(status=OK, statuses=statuses, take=take, chunk_of=chunk_of, chunks=chunks, chunk_first=[k["first"] for k in chunks],
                chunk_count=[k["count"] for k in chunks], coef_rel=coef_rel, pix_rel=pix_rel, out_bytes=out_bytes, plane_rel=plane_rel,
                row_bytes=rowb, rows=rows, rgb_rel=rgb_rel, rimg=rimg, scaled=scaled, wants=wants)


def skipped(plan, f, later, back):
    return later[f] != OK or not plan["out_bytes"][f] or bool(back and back[f])


def expected_runs(plan, form, later, back=None, host_reader_only=False):
    """-> the copies as (chunk, lo, bytes, row_stride, row_bytes, rows)"""
    reach = 4096 if form.scale == 1 and not form.resized and not host_reader_only else 1
    runs = []
    for j, k in enumerate(plan["chunks"]):
        run, last = None, None                                                  # [lo, hi] of the current run, its last position
        for t in range(k["first"], k["first"] + k["count"]):
            f = plan["take"][t]
            if skipped(plan, f, later, back):
                continue
            lo, hi = plan["pix_rel"][f], plan["pix_rel"][f] + plan["out_bytes"][f]
            if form.rgb is not None and form.strides and form.strides[f] > plan["row_bytes"][f]:
                if run:
                    runs.append((j, run[0], run[1] - run[0], 0, 0, 0))
                runs.append((j, lo, 0, form.strides[f], plan["row_bytes"][f], plan["rows"][f]))
                run = None                                                      # (the run's last position stays what it was)
                continue
            if run and t == last + 1 and run[1] <= lo < run[1] + reach:
                run[1] = hi
            else:
                if run:
                    runs.append((j, run[0], run[1] - run[0], 0, 0, 0))
                run = [lo, hi]
            last = t
        if run:
            runs.append((j, run[0], run[1] - run[0], 0, 0, 0))
    return runs


def check_runs_invariant(plan, form, runs, later, back=None):
    """no copy overlaps the record of a file that was skipped; the copies cover every byte of every file that was not (a file
    with room between its rows: every byte of its rows, and none between them)"""
    for j, k in enumerate(plan["chunks"]):
        copied = set()
        for (c, lo, nbytes, stride, rowb, rows) in runs:
            if c != j:
                continue
            pieces = [(lo + y * stride, rowb) for y in range(rows)] if rows else [(lo, nbytes)]
            for a, m in pieces:
                assert m > 0
                copied |= set(range(a, a + m))
        assert all(0 <= b < k["pix_hi"] - k["pix_lo"] for b in copied)          # inside the chunk's output slot
        for f in plan["take"][k["first"]:k["first"] + k["count"]]:
            lo = plan["pix_rel"][f]
            record = set(range(lo, lo + plan["out_bytes"][f]))
            if skipped(plan, f, later, back):
                assert not copied & record, f
            elif form.rgb is not None and form.strides and form.strides[f] > plan["row_bytes"][f]:
                written = {lo + y * form.strides[f] + x for y in range(plan["rows"][f]) for x in range(plan["row_bytes"][f])}
                assert copied & record == written, f
            else:
                assert record <= copied, f


# ---------------------------------------------------------------------------------------------------------------------------

def run_plan(harness, tmp_path, infos, status, offsets, cap, form, chunk_bytes=0, where=HOST, have_pixels=True, no_jpeg=(), later=None, back=None,
             host_reader_only=False):
    """-> what the harness printed, as a dict shaped like expected_plan's, with its copies under "runs" """
    n = len(infos)
    raw = struct.pack("<14q", n, chunk_bytes, where, cap, int(have_pixels), 0 if form.rgb is None else 1, form.rgb or 0,
                      0 if form.strides is None else 1, form.scale, 0 if form.sizes is None else 1, form.filter, int(form.heights),
                      int(host_reader_only), 0 if back is None else 1)
    raw += b"".join(bytes(i) for i in infos) + struct.pack("<%di" % n, *status) + bytes(0 if f in no_jpeg else 1 for f in range(n))
    raw += struct.pack("<%dQ" % n, *offsets)
    if form.strides is not None:
        raw += struct.pack("<%dQ" % n, *form.strides)
    if form.sizes is not None:
        raw += struct.pack("<%di" % n, *[s[0] for s in form.sizes]) + struct.pack("<%di" % n, *[s[1] for s in form.sizes])
    raw += struct.pack("<%di" % n, *(later if later is not None else [0] * n))
    if back is not None:
        raw += bytes(back)
    p = tmp_path / "set.bin"
    p.write_bytes(raw)
    r = subprocess.run([harness, str(p)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(chunks=[], rimg=[], scaled=[], runs=[])
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "status":
            out["status"] = int(w[1])
        elif w[0] == "chunk":
            out["chunks"].append(dict(zip(("first", "count", "coef_bytes", "pix_lo", "pix_hi", "plane_bytes", "rgb_bytes", "mid_bytes"), map(int, w[2:]))))
        elif w[0] in ("rimg", "scaled"):
            out[w[0]].append(list(map(int, w[2:])))
        elif w[0] == "run":
            out["runs"].append(tuple(map(int, w[1:])))
        elif w[0] == "wants":
            out["wants"] = dict(zip(("coef", "out", "plane", "rgb", "mid", "largest"), map(int, w[1:])))
        else:
            out[w[0]] = list(map(int, w[1:]))
    if out["status"] != OK:
        return dict(status=out["status"], statuses=out["statuses"])
    return out


def place(infos, form, gaps=None, align=64, start=0):
    """-> (offsets, cap): the records one after another, each on `align` bytes, gaps[f] bytes in front of record f"""
    at, offsets = start, []
    for f, i in enumerate(infos):
        at = up(at + (gaps or {}).get(f, 0), align)
        offsets.append(at)
        at += record_bytes(i, form, f)
    return offsets, at


def both(harness, tmp_path, infos, status, offsets, cap, form, later=None, back=None, host_reader_only=False, resize_status=None, **kw):
    """the harness and the rules side by side: every field of the plan, every copy, and the copies' invariant"""
    got = run_plan(harness, tmp_path, infos, status, offsets, cap, form, later=later, back=back, host_reader_only=host_reader_only, **kw)
    want = expected_plan(infos, status, offsets, cap, form, resize_status=resize_status, **kw)
    if want["status"] == OK:
        after = later if later is not None else [0] * len(infos)
        want["runs"] = []
        if kw.get("where", HOST) == HOST:                                       # (device output: nothing goes back)
            want["runs"] = expected_runs(want, form, after, back, host_reader_only)
            check_runs_invariant(want, form, got["runs"], after, back)
    assert got == want
    return got


@pytest.mark.parametrize("name", FORMS)
def test_one_chunk_and_a_cut_after_every_file(harness, tmp_path, infos, name):
    """chunk_bytes 0 = 64 MiB: one chunk; 1: every file above it, a chunk each.  Every ring size is the maximum over the chunks,
    chunk_first / chunk_count are the chunks'."""
    form = form_of(name)
    offsets, cap = place(infos, form)
    one = both(harness, tmp_path, infos, [0] * 5, offsets, cap, form)
    assert one["take"] == [0, 1, 2, 3, 4] and [k["count"] for k in one["chunks"]] == [5] and one["chunks"][0]["coef_bytes"] == sum(COEF_BYTES)
    each = both(harness, tmp_path, infos, [0] * 5, offsets, cap, form, chunk_bytes=1)
    assert [k["count"] for k in each["chunks"]] == [1] * 5 and each["coef_rel"] == [0] * 5 and each["pix_rel"] == [0] * 5
    for got in (one, each):
        ks, w = got["chunks"], got["wants"]
        assert w == dict(coef=max(k["coef_bytes"] for k in ks), out=max(k["pix_hi"] - k["pix_lo"] for k in ks),
                         plane=max(k["plane_bytes"] for k in ks), rgb=max(k["rgb_bytes"] for k in ks), mid=max(k["mid_bytes"] for k in ks),
                         largest=max(k["count"] for k in ks))
        assert got["chunk_first"] == [k["first"] for k in ks] and got["chunk_count"] == [k["count"] for k in ks]
        assert sum(got["chunk_count"]) == len(got["take"]) and got["chunk_first"] == [sum(got["chunk_count"][:j]) for j in range(len(ks))]
        assert (w["plane"] > 0) == (form.rgb is not None) and (w["rgb"] > 0) == (w["mid"] > 0) == form.resized
    assert each["wants"]["coef"] == 3072 and one["wants"]["largest"] == 5


@pytest.mark.parametrize("name", FORMS)
@pytest.mark.parametrize("chunk_bytes,counts", [(384 + 768 + 1024, [3, 1, 1]), (384 + 768 + 1024 - 1, [2, 1, 1, 1]), (3072, [3, 1, 1]),
                                                (3072 + 1536, [3, 2]), (3072 + 1536 - 1, [3, 1, 1])])
def test_a_cut_on_a_record_boundary_and_a_byte_short_of_it(harness, tmp_path, infos, name, chunk_bytes, counts):
    form = form_of(name)
    offsets, cap = place(infos, form)
    got = both(harness, tmp_path, infos, [0] * 5, offsets, cap, form, chunk_bytes=chunk_bytes)
    assert [k["count"] for k in got["chunks"]] == counts
    for k in got["chunks"]:
        assert k["count"] == 1 or k["coef_bytes"] <= chunk_bytes


@pytest.mark.parametrize("name", FORMS)
@pytest.mark.parametrize("bad", [0, 2, 4])
def test_a_file_that_arrives_with_a_status(harness, tmp_path, infos, name, bad):
    """first, middle, last: it is skipped with the code it came with, and needs no file"""
    form = form_of(name)
    offsets, cap = place(infos, form)
    status = [BAD_JPEG if f == bad else 0 for f in range(5)]
    got = both(harness, tmp_path, infos, status, offsets, cap, form, chunk_bytes=2000, no_jpeg=(bad,))
    assert got["statuses"] == status and got["chunk_of"][bad] == -1 and bad not in got["take"] and len(got["take"]) == 4
    assert got["out_bytes"][bad] == 0 and got["coef_rel"][bad] == 0


@pytest.mark.parametrize("name", FORMS)
def test_a_file_without_a_coefficient(harness, tmp_path, infos, name):
    """coef_count 0: it takes part, adds nothing to its chunk's coefficient record and closes no chunk"""
    form = form_of(name, 3)
    empty = copy_of(infos[1])
    empty.coef_count = 0
    files = [infos[0], empty, infos[2]]
    offsets, cap = place(files, form)
    got = both(harness, tmp_path, files, [0] * 3, offsets, cap, form, chunk_bytes=384)
    assert got["take"] == [0, 1, 2] and got["chunk_of"] == [0, 0, 1] and got["coef_rel"] == [0, 192, 0]
    assert got["chunks"][0]["coef_bytes"] == 384 and got["out_bytes"][1] > 0


@pytest.mark.parametrize("name", FORMS)
def test_host_and_device_output(harness, tmp_path, infos, name):
    """pix_rel and the output ring exist only for host memory; the resized images go to pix_rel there and to the caller's own
    offsets on the device"""
    form = form_of(name)
    offsets, cap = place(infos, form, start=4096)
    host = both(harness, tmp_path, infos, [0] * 5, offsets, cap, form, chunk_bytes=2000)
    dev = both(harness, tmp_path, infos, [0] * 5, offsets, cap, form, chunk_bytes=2000, where=DEVICE)
    assert dev["pix_rel"] == [0] * 5 and dev["wants"]["out"] == 0 and dev["runs"] == []
    assert host["wants"]["out"] > 0 and any(host["pix_rel"])
    assert {k: v for k, v in host.items() if k not in ("pix_rel", "wants", "rimg", "runs")} == {k: v for k, v in dev.items() if k not in ("pix_rel", "wants", "rimg", "runs")}
    if form.resized:
        assert [im[6] for im in dev["rimg"]] == offsets and [im[6] for im in host["rimg"]] == host["pix_rel"]


@pytest.mark.parametrize("name", FORMS)
def test_pixel_offsets_out_of_order(harness, tmp_path, infos, name):
    """pix_lo is the smallest offset of the chunk, rounded down to 8 -- not the first file's"""
    form = form_of(name)
    on8 = form.rgb is None and form.scale == 1                                  # (full-size planes lie on 8 bytes, everything else anywhere)
    at, offs = 16 if on8 else 13, [0] * 5
    for f in (3, 1, 4, 0, 2):                                                   # the order the records lie in
        offs[f] = at
        at = up(at + record_bytes(infos[f], form, f), 8 if on8 else 1)
    cap = max(offs[f] + record_bytes(infos[f], form, f) for f in range(5))
    got = both(harness, tmp_path, infos, [0] * 5, offs, cap, form)
    assert got["chunks"][0]["pix_lo"] == min(offs) // 8 * 8 != offs[0] // 8 * 8 and got["chunks"][0]["pix_hi"] == cap
    assert got["pix_rel"] == [o - min(offs) // 8 * 8 for o in offs]
    both(harness, tmp_path, infos, [0] * 5, offs, cap, form, chunk_bytes=2000)


def test_plane_alignment(harness, tmp_path, infos):
    """full-size planes at an offset that is no multiple of 8: HVC_E_ALIGNMENT for the call; the same offset at 1/2 size is taken"""
    offsets, cap = place(infos, Form())
    offsets[2] += 4
    got = both(harness, tmp_path, infos, [0] * 5, offsets, cap + 4, Form())
    assert got["status"] == ALIGNMENT
    assert both(harness, tmp_path, infos, [0] * 5, offsets, cap + 4, Form(scale=2))["status"] == OK
    assert both(harness, tmp_path, infos, [0] * 5, offsets, cap + 4, Form(rgb=0))["status"] == OK           # images lie anywhere too
    grey = copy_of(infos[2])                                                    # ... and planes of no bytes are nowhere
    grey.pixel_bytes = 0
    files = infos[:2] + [grey] + infos[3:]
    assert both(harness, tmp_path, files, [0] * 5, offsets, cap + 4, Form())["status"] == OK


@pytest.mark.parametrize("name", FORMS)
def test_the_end_of_the_buffer(harness, tmp_path, infos, name):
    """a record that ends exactly at pixel_cap is taken, one byte past it refused; an offset above pixel_cap is refused whatever
    the record (no wrap-around)"""
    form = form_of(name)
    offsets, cap = place(infos, form)
    assert both(harness, tmp_path, infos, [0] * 5, offsets, cap, form)["status"] == OK
    assert both(harness, tmp_path, infos, [0] * 5, offsets, cap - 1, form)["status"] == INVALID_ARG
    far = list(offsets)
    far[1] = cap + 8
    assert both(harness, tmp_path, infos, [0] * 5, far, cap, form)["status"] == INVALID_ARG
    far[1] = 2 ** 64 - 8                                                        # offset + bytes wraps around
    assert run_plan(harness, tmp_path, infos, [0] * 5, far, cap, form)["status"] == INVALID_ARG
    far[1] = cap                                                                # at the end itself: only a record of no bytes fits
    assert both(harness, tmp_path, infos, [0] * 5, far, cap, form)["status"] == INVALID_ARG


@pytest.mark.parametrize("name", FORMS)
def test_null_pixels(harness, tmp_path, infos, name):
    """no output buffer: HVC_E_INVALID_ARG as soon as one file has output bytes, fine where none has"""
    form = form_of(name)
    offsets, cap = place(infos, form)
    got = both(harness, tmp_path, infos, [0] * 5, offsets, cap, form, have_pixels=False)
    assert got["status"] == INVALID_ARG and got["statuses"] == [0] * 5
    nothing = []
    for i in infos:                                                             # files without a block, without a pixel
        e = copy_of(i)
        e.width = e.height = e.pixel_bytes = 0
        for k in range(4):
            e.layout[k].blocks_w = e.layout[k].blocks_h = 0
        nothing.append(e)
    sizes = form.but(sizes=[(0, 0)] * 5) if form.resized else form
    rs = {f: INVALID_ARG for f in range(5)} if form.resized else None           # (an image of no pixel is no image to resize)
    got = both(harness, tmp_path, nothing, [0] * 5, [0] * 5, 0, sizes, have_pixels=False, resize_status=rs)
    assert got["status"] == OK and got["out_bytes"] == [0] * 5
    assert got["take"] == ([] if form.resized else [0, 1, 2, 3, 4]) and got["runs"] == []


@pytest.mark.parametrize("name", FORMS)
def test_null_files(harness, tmp_path, infos, name):
    """a null jpegs[f] of a file that takes part ends the call; of one that arrives with a status it is never looked at"""
    form = form_of(name)
    offsets, cap = place(infos, form)
    assert both(harness, tmp_path, infos, [0] * 5, offsets, cap, form, no_jpeg=(3,))["status"] == INVALID_ARG
    assert both(harness, tmp_path, infos, [0, 0, 0, BAD_JPEG, 0], offsets, cap, form, no_jpeg=(3,))["status"] == OK


@pytest.mark.parametrize("layout", [0, 1])
def test_a_row_stride_below_the_row(harness, tmp_path, infos, layout):
    """one below tight: under the resized form the file's own status, else the call's error; tight itself is taken"""
    for form in (Form(rgb=layout), Form(rgb=layout, scale=2), Form(rgb=layout, sizes=OUT_SIZES)):
        w = form.sizes[2][0] if form.resized else output_of(infos[2], form)[0]
        tight = row_bytes(layout, w)
        ok = form.but(strides=[0, 0, tight, 0, 0])
        offsets, cap = place(infos, ok)
        assert both(harness, tmp_path, infos, [0] * 5, offsets, cap, ok)["statuses"] == [0] * 5
        short = form.but(strides=[0, 0, tight - 1, 0, 0])
        got = both(harness, tmp_path, infos, [0] * 5, offsets, cap, short)
        if form.resized:
            assert got["status"] == OK and got["statuses"] == [0, 0, INVALID_ARG, 0, 0] and got["take"] == [0, 1, 3, 4]
        else:
            assert got["status"] == INVALID_ARG


@pytest.mark.parametrize("name", ["rgb", "rgb_planar", "resized", "planes", "scale2"])
def test_a_sampling_that_is_not_rgbs(harness, tmp_path, infos, name):
    """the four-component file in the middle: its own status under an RGB form (and the statuses before a later call-level error
    stay); the planes forms take it"""
    form = form_of(name, 6)
    files = infos[:2] + [four_components(infos[0])] + infos[2:]
    if form.rgb is None:
        offsets, cap = place(files, form)
        got = both(harness, tmp_path, files, [0] * 6, offsets, cap, form)
        assert got["statuses"] == [0] * 6 and got["take"] == [0, 1, 2, 3, 4, 5]
        return
    offsets, cap = place(files, form)
    got = both(harness, tmp_path, files, [0] * 6, offsets, cap, form, chunk_bytes=2000)
    assert got["statuses"] == [0, 0, INVALID_ARG, 0, 0, 0] and got["take"] == [0, 1, 3, 4, 5] and got["chunk_of"][2] == -1
    late = both(harness, tmp_path, files, [0] * 6, offsets, cap, form, no_jpeg=(4,))
    assert late["status"] == INVALID_ARG and late["statuses"] == [0, 0, INVALID_ARG, 0, 0, 0]


def test_a_resize_target_that_is_refused(harness, tmp_path, infos):
    """what resize_image_status answers is the file's own status: a size below 1 (HVC_E_INVALID_ARG), 2^24 + 1 columns
    (HVC_E_TOO_LARGE: a side above 2^24) -- and the files around it lie where they lie without it"""
    for size, code in (((0, 5), INVALID_ARG), ((5, -1), INVALID_ARG), (((1 << 24) + 1, 1), TOO_LARGE)):
        sizes = list(OUT_SIZES)
        sizes[2] = size
        form = Form(rgb=0, sizes=sizes)
        offsets, cap = place(infos, Form(rgb=0, sizes=OUT_SIZES))
        got = both(harness, tmp_path, infos, [0] * 5, offsets, cap, form, resize_status={2: code})
        assert got["statuses"] == [0, 0, code, 0, 0] and got["take"] == [0, 1, 3, 4]
        without = both(harness, tmp_path, infos[:2] + infos[3:], [0] * 4, offsets[:2] + offsets[3:], cap, Form(rgb=0, sizes=sizes[:2] + sizes[3:]))
        assert got["chunks"] == without["chunks"] and got["wants"] == without["wants"]
        assert [v for f, v in enumerate(got["rgb_rel"]) if f != 2] == without["rgb_rel"]


def test_the_form_itself(harness, tmp_path, infos):
    """a scale that is none of 1, 2, 4, 8; the resized form without heights or with an unknown filter -- unless the set is empty"""
    offsets, cap = place(infos, Form())
    for scale in (0, 3, 16, -1):
        assert run_plan(harness, tmp_path, infos, [0] * 5, offsets, cap, Form(scale=scale))["status"] == INVALID_ARG
        assert expected_plan(infos, [0] * 5, offsets, cap, Form(scale=scale))["status"] == INVALID_ARG
    good = Form(rgb=0, sizes=OUT_SIZES)
    offsets, cap = place(infos, good)
    for bad in (good.but(heights=False), good.but(filter=3), good.but(filter=-1)):
        assert both(harness, tmp_path, infos, [0] * 5, offsets, cap, bad)["status"] == INVALID_ARG
        none = both(harness, tmp_path, [], [], [], 0, bad.but(sizes=[]))
        assert none["status"] == OK and none["take"] == [] and none["chunks"] == []
    for f in (BOX, BILINEAR, BICUBIC):
        assert both(harness, tmp_path, infos, [0] * 5, offsets, cap, good.but(filter=f))["status"] == OK


def test_empty_sets(harness, tmp_path, infos):
    empty = dict(coef=0, out=0, plane=0, rgb=0, mid=0, largest=0)
    offsets, cap = place(infos, Form())
    got = both(harness, tmp_path, infos, [BAD_JPEG] * 5, offsets, cap, Form(), have_pixels=False)
    assert got["status"] == OK and got["take"] == [] and got["chunks"] == [] and got["wants"] == empty and got["chunk_of"] == [-1] * 5
    got = both(harness, tmp_path, [four_components(infos[0])], [0], [0], 0, Form(rgb=1))
    assert got["status"] == OK and got["statuses"] == [INVALID_ARG] and got["take"] == [] and got["wants"] == empty


# ---------------------------------------------------------------------------------------------------------------------------
# the download runs

def three(infos):
    return [infos[0], infos[1], infos[0]]


@pytest.mark.parametrize("gap,joins", [(0, True), (8, True), (4095, True), (4096, False)])
def test_gaps_between_full_size_planes(harness, tmp_path, infos, gap, joins):
    """192 bytes of planes, then `gap` bytes, then 384: one copy while the gap is below 4096 bytes"""
    files = [copy_of(infos[0]), infos[1]]
    first = files[0].pixel_bytes = 193 if gap == 4095 else 192                  # (planes lie on 8 bytes: 193 + 4095 is a multiple of 8)
    offsets = [0, first + gap]
    got = both(harness, tmp_path, files, [0, 0], offsets, offsets[1] + 384, Form())
    end = offsets[1] + 384
    assert got["runs"] == ([(0, 0, end, 0, 0, 0)] if joins else [(0, 0, first, 0, 0, 0), (0, offsets[1], 384, 0, 0, 0)])


@pytest.mark.parametrize("kind", ["scale2", "resized", "host_reader_only"])
@pytest.mark.parametrize("gap", [0, 8, 4095, 4096])
def test_gaps_where_only_touching_records_join(harness, tmp_path, infos, kind, gap):
    form = form_of(kind, 2) if kind != "host_reader_only" else Form()
    files = [infos[0], infos[1]]
    if kind == "host_reader_only" and gap == 4095:
        files = [copy_of(infos[0]), infos[1]]
        files[0].pixel_bytes = 193
    first, second = record_bytes(files[0], form, 0), record_bytes(files[1], form, 1)
    offsets = [0, first + gap]
    got = both(harness, tmp_path, files, [0, 0], offsets, offsets[1] + second, form, host_reader_only=kind == "host_reader_only")
    assert got["runs"] == ([(0, 0, first + second, 0, 0, 0)] if gap == 0 else [(0, 0, first, 0, 0, 0), (0, offsets[1], second, 0, 0, 0)])


@pytest.mark.parametrize("name", FORMS)
@pytest.mark.parametrize("why", ["failed", "handed_back"])
def test_a_skipped_file_between_two_good_ones(harness, tmp_path, infos, name, why):
    """the middle file fails in its chunk (its later status), or the GPU reader hands it to the host reader (back[f] = 1): two
    runs, neither over its record -- however close the three records lie"""
    form = form_of(name, 3)
    files = three(infos)
    offsets, cap = place(files, form, align=8 if form.rgb is None and form.scale == 1 else 1)
    later, back = ([0, BAD_JPEG, 0], None) if why == "failed" else ([0, 0, 0], [0, 1, 0])
    got = both(harness, tmp_path, files, [0] * 3, offsets, cap, form, later=later, back=back)
    b = [record_bytes(files[f], form, f) for f in range(3)]
    assert got["runs"] == [(0, 0, b[0], 0, 0, 0), (0, offsets[2], b[2], 0, 0, 0)]
    whole = both(harness, tmp_path, files, [0] * 3, offsets, cap, form, back=[0, 0, 0] if why == "handed_back" else None)
    assert whole["runs"] == [(0, 0, cap, 0, 0, 0)]                            # all three good: they touch, one copy


@pytest.mark.parametrize("layout", [0, 1])
def test_a_file_with_room_between_its_rows(harness, tmp_path, infos, layout):
    """tight, padded, tight: the run so far, one 2-D copy of the padded image's rows (3 * height of them for the planar
    layout), then a new run -- which the file behind the padded one starts even where it touches"""
    files = three(infos)
    tight = row_bytes(layout, 16)
    form = Form(rgb=layout, strides=[0, tight + 5, 0])
    offsets, cap = place(files, form, align=1)
    got = both(harness, tmp_path, files, [0] * 3, offsets, cap, form)
    b = [record_bytes(files[f], form, f) for f in range(3)]
    assert b[1] == (rows_of(layout, 16) - 1) * (tight + 5) + tight
    assert got["runs"] == [(0, 0, b[0], 0, 0, 0), (0, offsets[1], 0, tight + 5, tight, 48 if layout else 16), (0, offsets[2], b[2], 0, 0, 0)]
    assert got["rows"] == [rows_of(layout, 8), rows_of(layout, 16), rows_of(layout, 8)]
    four = files + [infos[2]]                                                   # ... and the file after that joins the new run
    form = Form(rgb=layout, strides=[0, tight + 5, 0, 0])
    offsets, cap = place(four, form, align=1)
    got = both(harness, tmp_path, four, [0] * 4, offsets, cap, form)
    assert got["runs"][2:] == [(0, offsets[2], cap - offsets[2], 0, 0, 0)] and len(got["runs"]) == 3


@pytest.mark.parametrize("name", ["planes", "rgb", "scale2"])
def test_a_record_in_front_of_the_runs_end(harness, tmp_path, infos, name):
    """offsets out of order: the second file's record lies in front of the first's, so it starts a run of its own"""
    form = form_of(name, 2)
    files = [infos[0], infos[1]]
    b = [record_bytes(files[f], form, f) for f in range(2)]
    offsets = [up(b[1], 8), 0]
    got = both(harness, tmp_path, files, [0] * 2, offsets, offsets[0] + b[0], form)
    assert got["runs"] == [(0, offsets[0], b[0], 0, 0, 0), (0, 0, b[1], 0, 0, 0)] and got["chunks"][0]["pix_lo"] == 0
