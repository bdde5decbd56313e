"""Mixed batches at 1/2, 1/4, 1/8 size on the GPU: hvc_decode_frames_mixed_scaled (frames of different geometry and tables in
one launch of k_decode_mixed_scaled), hvc_jpeg_decode_batch_mixed_scaled and hvc_jpeg_decode_batch_mixed_scaled_rgb.  The
expected bytes come from the numpy definition (tools/scaled_reference.py, tools/rgb_reference.py) and from the
single-geometry entry points -- hvc_decode_frames_scaled, hvc_jpeg_decode_scaled, hvc_jpeg_decode_scaled_rgb -- called on
each frame or file alone; never from the code under test.  Every comparison is exact equality; where a whole buffer is
compared, what lies between rows, planes and records must keep its fill."""
import ctypes as C
import os
import pathlib
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden_bytes
from helpers import jpeg_optimised_tables
from oracle import orc
from test_gpu_scaled import definition_of_file, guard_record, sampling_of
from test_host_entropy import UNUSUAL_SAMPLINGS, unusual_sampling_file
from test_mixed_rgb_plan import FACTORS, UNCONVERTIBLE
from test_restart_intervals import QT, random_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rgb_reference as rgb_ref  # noqa: E402
import scaled_reference as sr  # noqa: E402

pytestmark = pytest.mark.gpu

SCALES = (2, 4, 8)
FILL = 0xA5
PLACEMENTS = ("tight", "dwords", "bytes")


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture()
def ctx(hvc):
    c = hvc.Context(0)
    yield c
    c.close()


def table(chroma, quality):
    return orc.quant_scale(orc.quant_chroma() if chroma else orc.quant_luma(), quality).astype(np.uint16)


def up(v, a):
    return -(-v // a) * a


# ---------------------------------------------------------------------------
# frames of different geometry in one launch

def ordinary_blocks(seed, nblk):
    """sparse small coefficients: with the tables used here every block stays inside the int32 guard"""
    rng = np.random.default_rng(seed)
    c = rng.integers(-12, 13, size=(nblk, 64))
    c *= rng.random(size=c.shape) < 0.3
    c[:, 0] = rng.integers(-60, 61, size=nblk)
    return c.astype(np.int16)


def frame_of(hvc, planes, tables, seed=0, coefs=None):
    """planes: (blocks_w, blocks_h, qtab) each; tables: arrays of 64; coefs: per plane [blocks][64] (default: ordinary_blocks)
    -> dict(info (blocks, tables, coefficient offsets), planes, tables, coefs (the tight record), blocks (per plane))"""
    info = hvc.hvc.JpegInfo()
    info.n_comp, info.n_qtabs = len(planes), len(tables)
    for t, q in enumerate(tables):
        for k in range(64):
            info.qtabs[t][k] = int(q[k])
    rec, blocks, off = [], [], 0
    for i, (bw, bh, qt) in enumerate(planes):
        L = info.layout[i]
        L.blocks_w, L.blocks_h, L.qtab, L.coef_offset = bw, bh, qt, off
        b = ordinary_blocks(seed + i, bw * bh) if coefs is None else np.asarray(coefs[i], dtype=np.int16).reshape(bw * bh, 64)
        blocks.append(b)
        rec.append(b.reshape(-1))
        off += bw * bh * 64
    info.coef_count = off
    return dict(info=info, planes=planes, tables=tables, coefs=np.concatenate(rec), blocks=blocks)


@pytest.fixture(scope="module")
def shapes(hvc):
    ql, qc = table(0, 75), table(1, 75)
    return [
        frame_of(hvc, [(1, 1, 0)], [ql], 11),                                   # one block
        frame_of(hvc, [(8, 8, 0), (4, 4, 1), (4, 4, 1)], [ql, qc], 21),         # 64 / 16 / 16 blocks
        frame_of(hvc, [(9, 8, 0), (9, 8, 1), (9, 8, 1)], [ql, qc], 31),         # 72 blocks: a unit boundary; bw odd
        frame_of(hvc, [(1, 257, 0)], [qc], 41),                                 # bw = 1: a workgroup boundary, nothing ever joins
        frame_of(hvc, [(5, 13, 0)], [ql], 45),                                  # 65 blocks; N = 1: stride 5
        frame_of(hvc, [(6, 11, 0)], [qc], 47),                                  # N = 1: stride 6; N = 2: stride 12
        frame_of(hvc, [(66, 33, 0), (33, 33, 1), (33, 33, 1)], [ql, qc], 51),   # 4:2:2
        frame_of(hvc, [(4, 3, 0), (0, 3, 1), (2, 2, 1)], [ql, qc], 61),         # a zero-size component
    ]


def place(hvc, frames, n, placement):
    """-> (infos with the scaled planes placed, pixel offsets, buffer size).  tight: hvc_jpeg_scaled_info's planes; dwords:
    strides rounded up to 4, plane offsets on 4; bytes: as dwords with every record one byte further.  Records lie 8-aligned
    (bytes: + 1) with sentinel bytes before, between and behind them."""
    infos, po, at = [], [], 8
    for fr in frames:
        info = type(fr["info"]).from_buffer_copy(fr["info"])
        off = 0
        for i, (bw, bh, _) in enumerate(fr["planes"]):
            L = info.layout[i]
            L.stride = bw * n if placement == "tight" else up(bw * n, 4)
            L.plane_offset = off
            off += L.stride * bh * n
            if placement != "tight":
                off = up(off, 4) + 4
        info.pixel_bytes = off
        infos.append(info)
        po.append(at + (1 if placement == "bytes" else 0))
        at = up(at + off + 3, 8) + 8
    return infos, po, at + 16


def want_buffer(frames, infos, po, size, n):
    """the whole buffer by the definition (FILL outside the planes) and the number of blocks outside the int32 guard"""
    out = np.full(size, FILL, dtype=np.uint8)
    wide = 0
    for fr, info, off in zip(frames, infos, po):
        for i, (bw, bh, qt) in enumerate(fr["planes"]):
            if not bw * bh:
                continue
            L = info.layout[i]
            plane = sr.scaled_plane(fr["blocks"][i], fr["tables"][qt], bw, bh, n)
            wide += int(np.count_nonzero(~sr.takes_int32_path(fr["blocks"][i], fr["tables"][qt], n)))
            rows = off + L.plane_offset + np.arange(bh * n)[:, None] * L.stride + np.arange(bw * n)[None, :]
            out[rows] = plane
    return out, wide


def run_frames(ctx, frames, infos, po, size, scale, device):
    import torch
    co = np.concatenate([[0], np.cumsum([fr["coefs"].size for fr in frames])])[:len(frames)].tolist()
    coefs = np.concatenate([fr["coefs"] for fr in frames] + [np.zeros(64, np.int16)])
    pixels = np.full(size, FILL, dtype=np.uint8)
    if device:
        d_c, d_p = torch.from_numpy(coefs).cuda(), torch.from_numpy(pixels).cuda()
        torch.cuda.synchronize()
        ctx.decode_frames_mixed_scaled(d_c, co, infos, scale, d_p, po)
        ctx.synchronize()
        pixels = d_p.cpu().numpy()
    else:
        ctx.decode_frames_mixed_scaled(coefs, co, infos, scale, pixels, po)
    return pixels


def alone(ctx, fr, info, scale):
    """hvc_decode_frames_scaled on that frame alone (host memory), in the same placement"""
    specs = [dict(blocks_w=bw, blocks_h=bh, qtab=qt, coef_offset=info.layout[i].coef_offset, plane_offset=info.layout[i].plane_offset,
                  stride=info.layout[i].stride) for i, (bw, bh, qt) in enumerate(fr["planes"])]
    out = np.full(max(info.pixel_bytes, 8), FILL, dtype=np.uint8)
    ctx.decode_frames_scaled(fr["coefs"], fr["coefs"].size, np.stack(fr["tables"]), specs, 1, scale, out, out.size)
    return out[:info.pixel_bytes]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("scale", SCALES)
def test_records_of_different_geometry(ctx, hvc, shapes, scale, placement, reverse, device):
    n = 8 // scale
    frames = shapes[::-1] if reverse else shapes
    infos, po, size = place(hvc, frames, n, placement)
    want, wide = want_buffer(frames, infos, po, size, n)
    got = run_frames(ctx, frames, infos, po, size, scale, device)
    assert np.array_equal(got, want)                                           # == the definition, sentinels included
    assert wide == 0 and ctx.last_wide_blocks() == 0
    if not reverse and not device:                                             # == hvc_decode_frames_scaled on that frame alone
        for fr, info, off in zip(frames, infos, po):
            assert np.array_equal(got[off:off + info.pixel_bytes], alone(ctx, fr, info, scale))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("placement", ["tight", "dwords"])
@pytest.mark.parametrize("scale", SCALES)
def test_both_sides_of_the_guard_in_adjacent_frames(ctx, hvc, scale, placement, device):
    """guard_record's blocks (both sides of the int32 guard, the int16 extremes, tables of 255 / 65535 / 1) beside ordinary
    frames and a table with an entry of 300: the bytes are the definition's, the count is the guard's"""
    n = 8 // scale
    q, planes, coefs = guard_record(n)
    per_plane = coefs.reshape(3, 36, 64)
    q300 = table(0, 50).copy()
    q300[5] = 300
    frames = [frame_of(hvc, [(3, 3, 0)], [table(0, 75)], 7),
              frame_of(hvc, planes, list(q), coefs=per_plane),
              frame_of(hvc, [(7, 5, 0), (5, 3, 1)], [q300, table(1, 20)], 9),
              frame_of(hvc, planes, list(q), coefs=per_plane[:, ::-1, ::1]),   # the blocks in reverse order
              frame_of(hvc, [(2, 5, 0)], [table(1, 90)], 8)]
    infos, po, size = place(hvc, frames, n, placement)
    want, wide = want_buffer(frames, infos, po, size, n)
    got = run_frames(ctx, frames, infos, po, size, scale, device)
    assert np.array_equal(got, want)
    assert ctx.last_wide_blocks() == wide
    assert (wide > 40) == (n > 1)                                              # both branches are taken (N = 1 has one)
    assert n == 1 or wide < sum(fr["coefs"].size for fr in frames) // 64 - 40


def test_a_set_without_a_block_launches_nothing(ctx, hvc):
    fr = frame_of(hvc, [(0, 3, 0), (2, 0, 0)], [table(0, 50)], 1)
    for scale in SCALES:
        ctx.decode_frames_mixed_scaled(np.zeros(64, np.int16), [0], [fr["info"]], scale, np.zeros(8, np.uint8), [0])
        ctx.decode_frames_mixed_scaled(np.zeros(64, np.int16), [], [], scale, np.zeros(8, np.uint8), [])


def test_scale_1_is_decode_frames_mixed(ctx, hvc, shapes):
    frames = shapes[:4]
    infos, po, at = [], [], 0
    for fr in frames:
        info = type(fr["info"]).from_buffer_copy(fr["info"])
        off = 0
        for i, (bw, bh, _) in enumerate(fr["planes"]):
            info.layout[i].stride, info.layout[i].plane_offset = bw * 8, off
            off += bw * bh * 64
        info.pixel_bytes = off
        infos.append(info)
        po.append(at)
        at += up(off, 256)
    co = np.concatenate([[0], np.cumsum([fr["coefs"].size for fr in frames])])[:len(frames)].tolist()
    coefs = np.concatenate([fr["coefs"] for fr in frames])
    a, b = np.full(at, FILL, dtype=np.uint8), np.full(at, FILL, dtype=np.uint8)
    ctx.decode_frames_mixed(coefs, co, infos, a, po)
    ctx.decode_frames_mixed_scaled(coefs, co, infos, 1, b, po)
    assert np.array_equal(a, b) and not (a == FILL).all()
    with pytest.raises(hvc.hvc.HvcError) as e:                                 # ... with its alignment rule
        ctx.decode_frames_mixed_scaled(coefs, co[:1], infos[:1], 1, b, [4])
    assert e.value.code == -4


# ---------------------------------------------------------------------------
# files

@pytest.fixture(scope="module")
def file_set():
    files = [golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")]
    for si in (0, 1, 3, 4, 6, 8, 9, 10, 11):
        files.append(unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 40, 24, 100 * si + 40)[0])
    for si in (2, 5, 7, 8, 10):
        files.append(unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 97, 51, 100 * si + 97)[0])
    for si in (3, 9):
        files.append(unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 70, 38, 100 * si + 70)[0])
    for seed in (1, 2):   # one geometry, different optimised Huffman tables (fitted to each file's own symbols)
        files.append(jpeg_optimised_tables(96, 64, 420, QT, random_record([(2, 2), (1, 1), (1, 1)], 96, 64, seed)[0]))
    return files


_WANT = {}


def want_file(hvc, data, scale, restart=False):
    """(scaled info, the planes by the numpy definition), computed once per file, scale and setting"""
    key = (data, scale, restart)
    if key not in _WANT:
        _WANT[key] = definition_of_file(hvc, data, scale, restart)
    return _WANT[key]


def check_files(hvc, files, results, scale, skip=(), restart=False):
    for f, (data, (status, info, planes)) in enumerate(zip(files, results)):
        if f in skip:
            continue
        sinfo, want = want_file(hvc, data, scale, restart)
        assert status == 0 and len(planes) == len(want), f
        assert bytes(info) == bytes(sinfo), f
        for i, (got, w) in enumerate(zip(planes, want)):
            got = got.cpu().numpy() if hasattr(got, "cpu") else got
            assert np.array_equal(got, w), (f, i)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("threads", [1, 2])
@pytest.mark.parametrize("scale", SCALES)
def test_files_of_mixed_sizes_samplings_and_tables(ctx, hvc, file_set, scale, threads, device):
    coef_bytes = [2 * hvc.hvc.jpeg_read_header(f).coef_count for f in file_set]
    chunk = 40000                                  # Mouse480 alone is larger (its ring slot grows); the others fill several chunks
    assert max(coef_bytes) > chunk
    chunks, cur, cnt, largest = 0, 0, 0, 0         # the chunking rule, restated
    for b in coef_bytes:
        if chunks == 0 or (cnt > 0 and cur + b > chunk):
            chunks, cur, cnt = chunks + 1, 0, 0
        cur, cnt = cur + b, cnt + 1
        largest = max(largest, cnt)
    assert chunks >= 3
    results = ctx.jpeg_decode_batch_mixed_scaled(file_set, scale, threads=threads, chunk_bytes=chunk, device=device)
    check_files(hvc, file_set, results, scale)
    st = ctx.last_batch_stats
    assert (st.chunks, st.frames_per_chunk, st.coef_bytes, st.threads) == (chunks, largest, sum(coef_bytes), threads)
    assert st.entropy_ms_sum > 0
    if threads == 1 and not device:                # == hvc_jpeg_decode_scaled of every file alone
        for data, (_, info, planes) in zip(file_set, results):
            i1, px = ctx.jpeg_decode_scaled(data, scale)
            assert bytes(i1) == bytes(info)
            for a, b in zip(planes, i1.planes(px)):
                assert np.array_equal(a, b)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("scale", [2, 8])
def test_whole_buffer_with_sentinels(ctx, hvc, file_set, scale, device):
    """records on 256 bytes with room between them: no byte outside the good files' records is written, in host and in device
    memory"""
    import torch
    files = file_set[:1] + file_set[2:12]
    lay = hvc.hvc.jpeg_mixed_scaled_layout(files, scale, 256)
    want = np.full(lay.total_bytes + 16, FILL, dtype=np.uint8)
    for f, data in enumerate(files):
        sinfo, planes = want_file(hvc, data, scale)
        off = lay.pixel_offsets[f]
        want[off:off + sinfo.pixel_bytes] = np.concatenate([p.reshape(-1) for p in planes])
    pixels = np.full(lay.total_bytes + 16, FILL, dtype=np.uint8)
    if device:
        pixels = torch.from_numpy(pixels).cuda()
    ctx.jpeg_decode_batch_mixed_scaled(files, scale, threads=2, chunk_bytes=20000, device=device, layout=lay, pixels=pixels)
    got = pixels.cpu().numpy() if device else pixels
    assert np.array_equal(got, want)
    assert any(lay.pixel_offsets[f + 1] > lay.pixel_offsets[f] + lay.scaled[f].pixel_bytes for f in range(len(files) - 1))   # there ARE gaps


def broken_files(hvc, file_set):
    info = hvc.hvc.jpeg_read_header(file_set[1])
    # cut in its scan (one-bits follow the cut, which no Huffman table has a code for: tests/test_gpu_mixed.py)
    cut = file_set[1][:info.ecs_offset + 2000] + b"\xff\x00" * 64 + b"\xff\xd9"
    with pytest.raises(hvc.hvc.HvcError) as e:
        hvc.hvc.jpeg_entropy_decode(cut)
    cut_code = e.value.code
    garbage = np.random.Generator(np.random.PCG64(3)).integers(0, 256, size=3000, dtype=np.uint8).tobytes()
    rec = np.zeros(3 * 64 * 64, dtype=np.int64).reshape(3, 64, 64)
    rec[0, :, 0] = 2047 * (np.arange(64) + 1)                                  # absolute DCs up to 131 008: beyond int16
    wide_dc = jpeg_optimised_tables(64, 64, 444, np.stack([table(0, 75), table(1, 75)]), rec.reshape(-1), table_sets=2)
    return {3: (cut, cut_code), 9: (garbage, None), 14: (wide_dc, -5)}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("scale", [2, 8])
def test_a_failing_file_stops_nobody_else(ctx, hvc, file_set, scale, device):
    import torch
    files = list(file_set)
    bad = broken_files(hvc, file_set)
    for at in sorted(bad):
        files.insert(at, bad[at][0])
    lay = hvc.hvc.jpeg_mixed_scaled_layout(files, scale)
    assert lay.status[9] != 0 and lay.status[3] == 0 and lay.status[14] == 0
    pixels = np.full(lay.total_bytes, FILL, dtype=np.uint8)
    if device:
        pixels = torch.from_numpy(pixels).cuda()
    results = ctx.jpeg_decode_batch_mixed_scaled(files, scale, threads=2, chunk_bytes=60000, device=device, layout=lay, pixels=pixels)
    check_files(hvc, files, results, scale, skip=bad)
    assert results[3][0] == bad[3][1] != 0 and results[14][0] == -5 and results[9][0] == lay.status[9] and results[9][2] is None
    host = pixels.cpu().numpy() if device else pixels
    for at in (3, 14):                                                         # their records keep the sentinel
        off = lay.pixel_offsets[at]
        assert lay.scaled[at].pixel_bytes > 0 and (host[off:off + lay.scaled[at].pixel_bytes] == FILL).all(), at
    again = ctx.jpeg_decode_batch_mixed_scaled(file_set[:6], scale, threads=2, device=device)   # and the context decodes another batch
    check_files(hvc, file_set[:6], again, scale)


@pytest.fixture(scope="module")
def marked_file():
    """one file with DRI whose reading by the model (the first interval only) stays inside int16: tests/test_gpu_mixed.py"""
    rec, _ = random_record([(2, 2), (1, 1), (1, 1)], 200, 72, 9)
    blocks = rec.reshape(-1, 64).copy()
    rng = np.random.Generator(np.random.PCG64(1))
    blocks[:, 0] = 40
    blocks[rng.integers(0, len(blocks), size=30), 0] = rng.integers(-200, 200, size=30)
    blocks[rng.random(len(blocks)) < 0.6, 1:] = 0
    return jpeg_optimised_tables(200, 72, 420, QT, blocks.reshape(-1), restart_interval=5)


@pytest.mark.parametrize("scale", SCALES)
def test_restart_markers(ctx, hvc, marked_file, scale):
    files = [golden_bytes("mini.jpg"), marked_file]
    planes_of = {}
    for honour in (False, True):
        ctx.set_restart_markers(honour)
        try:
            results = ctx.jpeg_decode_batch_mixed_scaled(files, scale, threads=2)
            assert [r[0] for r in results] == [0, 0]
            check_files(hvc, files, results, scale, restart=honour)            # == the definition over the reader's record
            for f, (_, info, planes) in zip(files, results):
                i1, px = ctx.jpeg_decode_scaled(f, scale)                      # the same setting, one file at a time
                for a, b in zip(planes, i1.planes(px)):
                    assert np.array_equal(a, b)
            planes_of[honour] = np.concatenate([p.reshape(-1) for p in results[1][2]])
            if scale == 4:
                rgb = ctx.jpeg_decode_batch_mixed_scaled_rgb(files, scale, threads=2)
                assert np.array_equal(rgb[1][2], ctx.jpeg_decode_scaled_rgb(marked_file, scale)[1])
        finally:
            ctx.set_restart_markers(False)
    assert not np.array_equal(planes_of[False], planes_of[True])


# ---------------------------------------------------------------------------
# files to RGB

@pytest.fixture(scope="module")
def rgb_files():
    """4:2:0 / 4:2:2 / 4:4:4 / grey at sizes whose scaled sizes are odd, and 4:1:1 files in between (kind 0: no RGB image)"""
    files, kinds = [golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")], [420, 420]
    for (w, h) in ((70, 38), (97, 51), (45, 53)):
        for kind in (420, 422, 444, 400):
            files.append(unusual_sampling_file(FACTORS[kind], w, h, 1000 + kind + w)[0])
            kinds.append(kind)
        files.append(unusual_sampling_file(UNCONVERTIBLE[0], w, h, 2000 + w)[0])   # 4:1:1
        kinds.append(0)
    return files, kinds


_ALONE = {}


def rgb_alone(ctx, data, scale, layout):
    key = (data, scale, layout)
    if key not in _ALONE:
        _ALONE[key] = ctx.jpeg_decode_scaled_rgb(data, scale, layout)[1]
    return _ALONE[key]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout,row_align", [("interleaved", 1), ("interleaved", 8), ("planar", 1), ("planar", 8)])
@pytest.mark.parametrize("scale", SCALES)
def test_files_to_rgb(ctx, hvc, rgb_files, scale, layout, row_align, device):
    import torch
    files, kinds = rgb_files
    lay = hvc.hvc.jpeg_mixed_scaled_rgb_layout(files, scale, layout, 8, row_align)
    rgb = np.full(lay.total_bytes + 16, FILL, dtype=np.uint8)
    if device:
        rgb = torch.from_numpy(rgb).cuda()
    results = ctx.jpeg_decode_batch_mixed_scaled_rgb(files, scale, threads=2, chunk_bytes=40000, device=device, rgb_layout=lay, rgb=rgb)
    assert ctx.last_batch_stats.chunks >= 3
    host = rgb.cpu().numpy() if device else rgb
    written = np.zeros(host.size, dtype=bool)
    end = 0
    for f, (data, kind, (status, info, image)) in enumerate(zip(files, kinds, results)):
        if kind == 0:                                                          # 4:1:1: status -1, no room, nothing touched
            assert status == -1 and image is None and lay.status[f] == -1 and lay.rgb_offsets[f] >= end, f
            continue
        assert status == 0, f
        sinfo, planes = want_file(hvc, data, scale)
        assert (info.width, info.height) == (sinfo.width, sinfo.height)
        image = image.cpu().numpy() if hasattr(image, "cpu") else image
        assert np.array_equal(image, rgb_alone(ctx, data, scale, layout)), f  # == hvc_jpeg_decode_scaled_rgb of the file alone
        p = planes + [None, None]                                              # == the colour definition over the definition's planes
        want = rgb_ref.planes_to_rgb(p[0], p[1], p[2], sampling_of(sinfo), sinfo.width, sinfo.height, layout)
        assert np.array_equal(image, want), f
        hvc.hvc.rgb_view(written, lay.rgb_offsets[f], lay.rgb_row_strides[f], info.width, info.height, layout)[...] = True
        end = lay.rgb_offsets[f] + lay.rgb_row_strides[f] * info.height * (3 if layout == "planar" else 1)
    assert (host[~written] == FILL).all()                                      # between rows, between records, behind the last


def test_errors(ctx, hvc, shapes):
    L = hvc.lib()
    files = [golden_bytes("mini.jpg"), unusual_sampling_file(FACTORS[422], 70, 38, 5)[0]]
    n = len(files)
    out = np.full(1 << 16, FILL, dtype=np.uint8)
    st = hvc.hvc.BatchStats()
    lay = hvc.hvc.jpeg_mixed_scaled_layout(files, 2, 8)
    rlay = hvc.hvc.jpeg_mixed_scaled_rgb_layout(files, 2, "interleaved", 8, 1)
    fr = shapes[1]
    infos, po, size = place(hvc, [fr], 4, "tight")
    arr, co, pos = (hvc.hvc.JpegInfo * 1)(*infos), (C.c_size_t * 1)(0), (C.c_size_t * 1)(*po)
    tot = C.c_size_t(0)

    def status_of(l):
        return (C.c_int * n)(*l.status)
    calls = {
        "layout": lambda s: L.hvc_jpeg_mixed_scaled_layout(lay.ptrs, lay.sizes, n, s, 8, (hvc.hvc.JpegInfo * n)(), (hvc.hvc.JpegInfo * n)(),
                                                           (C.c_int * n)(), (C.c_size_t * n)(), C.byref(tot)),
        "rgb_layout": lambda s: L.hvc_jpeg_mixed_scaled_rgb_layout(lay.ptrs, lay.sizes, n, s, 0, 8, 1, (hvc.hvc.JpegInfo * n)(),
                                                                   (hvc.hvc.JpegInfo * n)(), (C.c_int * n)(), (C.c_size_t * n)(),
                                                                   (C.c_size_t * n)(), C.byref(tot)),
        "frames": lambda s: L.hvc_decode_frames_mixed_scaled(ctx._h, fr["coefs"].ctypes.data, co, arr, 1, s, out.ctypes.data, pos, 0),
        "batch": lambda s, cap=out.size: L.hvc_jpeg_decode_batch_mixed_scaled(ctx._h, lay.ptrs, lay.sizes, n, 2, 0, s, lay.infos, status_of(lay),
                                                                             lay.pixel_offsets, out.ctypes.data, cap, 0, C.byref(st)),
        "batch_rgb": lambda s, cap=out.size: L.hvc_jpeg_decode_batch_mixed_scaled_rgb(ctx._h, rlay.ptrs, rlay.sizes, n, 2, 0, s, rlay.infos,
                                                                                     status_of(rlay), rlay.rgb_offsets, rlay.rgb_row_strides,
                                                                                     out.ctypes.data, cap, 0, 0, C.byref(st)),
    }
    for name, call in calls.items():                                           # a scale_denom that is none of 1, 2, 4, 8
        for s in (0, 3, 16, -2):
            assert call(s) == -1, (name, s)
    assert (out == FILL).all()
    ctx.set_arithmetic("hardcaml")                                             # no RTL form: refused, output untouched
    try:
        for name in ("frames", "batch", "batch_rgb"):
            for s in SCALES:
                assert calls[name](s) == -1, (name, s)
    finally:
        ctx.set_arithmetic("model")
    assert (out == FILL).all()
    assert calls["batch"](2, lay.total_bytes - 1) == -1                        # a pixel_cap / rgb_cap one byte short
    assert calls["batch_rgb"](2, rlay.total_bytes - 1) == -1
    assert (out == FILL).all()
    assert calls["batch"](2, lay.total_bytes) == 0 and not (out[:lay.total_bytes] == FILL).all() and (out[lay.total_bytes:] == FILL).all()
    assert calls["batch_rgb"](2, rlay.total_bytes) == 0 and calls["frames"](2) == 0
    narrow = type(infos[0]).from_buffer_copy(infos[0])                         # a stride below the row
    narrow.layout[0].stride -= 1
    assert L.hvc_decode_frames_mixed_scaled(ctx._h, fr["coefs"].ctypes.data, co, (hvc.hvc.JpegInfo * 1)(narrow), 1, 2, out.ctypes.data, pos, 0) == -1


def test_profiling_brackets_the_scaled_mixed_kernel(ctx, hvc, shapes):
    infos, po, size = place(hvc, shapes, 4, "tight")
    ctx.set_profiling(True)
    try:
        run_frames(ctx, shapes, infos, po, size, 2, True)
        ms = ctx.last_kernel_ms()
    finally:
        ctx.set_profiling(False)
    assert 0 < ms < 50


def test_cli_decode_frames_scaled(tmp_path, capsys):
    from video_coding_amd.__main__ import main
    golden = pathlib.Path(GOLDEN)
    third = tmp_path / "third.jpg"
    third.write_bytes(unusual_sampling_file(FACTORS[422], 97, 51, 4)[0])
    ins = [golden / "mini.jpg", golden / "Mouse480.jpg", third]
    for flags, ext in (([], ".yuv"), (["-rgb"], ".ppm")):
        out = tmp_path / ("out" + ext[1:])
        main(["model", "decode", "frames", str(out)] + [str(p) for p in ins] + ["-scale", "4"] + flags)
        for p in ins:
            one = tmp_path / (p.stem + "_one" + ext)
            main(["model", "decode", "frame", str(p), str(one), "-scale", "4"] + flags)
            assert (out / (p.stem + ext)).read_bytes() == one.read_bytes(), p
    broken = tmp_path / "broken.jpg"
    broken.write_bytes(golden_bytes("mini.jpg")[:100])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        main(["model", "decode", "frames", str(tmp_path / "out2"), str(ins[0]), str(broken), "-scale", "4"])
    assert e.value.code == 1 and "broken.jpg" in capsys.readouterr().err
    assert (tmp_path / "out2" / "mini.yuv").read_bytes() == (tmp_path / "outyuv" / "mini.yuv").read_bytes()


def test_the_measured_kernels_are_the_parents(hvc):
    """csrc/hvc_mixed_scaled.hip and csrc/hvc_scaled_dev.h are files of their own: the kernel id the counters are keyed on stays"""
    assert hvc.hvc.kernel_source_id() == hvc.hvc.kernel_build_id() == "b746d7b6f0f2"
