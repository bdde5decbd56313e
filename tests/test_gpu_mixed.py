"""Mixed batches on the GPU: hvc_decode_frames_mixed (frames of different geometry and tables in one launch of k_decode_mixed)
and hvc_jpeg_decode_batch_mixed (files of different sizes, samplings and tables in one call) against the single-geometry
entry points -- hvc_decode_frames, hvc_jpeg_decode -- and the model restatement, byte for byte."""
import pathlib

import numpy as np
import pytest

from conftest import GOLDEN, golden_bytes
from helpers import jpeg_optimised_tables, synth_coefs
from oracle import orc
from test_host_entropy import UNUSUAL_SAMPLINGS, unusual_sampling_file
from test_restart_intervals import QT, random_record

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


def table(chroma, quality):
    return orc.quant_scale(orc.quant_chroma() if chroma else orc.quant_luma(), quality).astype(np.uint16)


def make_frame(planes, tables, seed, coefs=None):
    """planes: (blocks_w, blocks_h, qtab) each; tables: arrays of 64 -> dict(info, coefs (the tight record), want (the
    restatement's tight pixel record))"""
    import video_coding_amd as hvc
    info = hvc.hvc.JpegInfo()
    info.n_comp, info.n_qtabs = len(planes), len(tables)
    for t, q in enumerate(tables):
        for k in range(64):
            info.qtabs[t][k] = int(q[k])
    rec, want, off = [], [], 0
    for i, (bw, bh, qt) in enumerate(planes):
        L = info.layout[i]
        L.blocks_w, L.blocks_h, L.qtab, L.coef_offset, L.plane_offset, L.stride = bw, bh, qt, off, off, bw * 8
        if bw * bh:
            c = synth_coefs(seed + i, bh, bw, tables[qt])[0] if coefs is None else coefs[i]
            rec.append(np.ascontiguousarray(c, dtype=np.int16).reshape(-1))
            want.append(orc.dequant_idct_recon(rec[-1], tables[qt], bw, bh))
        off += bw * bh * 64
    info.coef_count = info.pixel_bytes = off
    return dict(info=info, planes=planes, tables=tables, coefs=np.concatenate(rec) if rec else np.zeros(0, np.int16),
                want=np.concatenate(want) if want else np.zeros(0, np.uint8))


def alone(ctx, fr):
    """hvc_decode_frames on that frame alone (host memory)"""
    specs = [dict(blocks_w=bw, blocks_h=bh, qtab=qt, coef_offset=fr["info"].layout[i].coef_offset,
                  plane_offset=fr["info"].layout[i].plane_offset, stride=bw * 8) for i, (bw, bh, qt) in enumerate(fr["planes"])]
    out = np.full(max(fr["want"].size, 8), 0x5A, dtype=np.uint8)
    ctx.decode_frames(fr["coefs"] if fr["coefs"].size else np.zeros(64, np.int16), fr["info"].coef_count, np.stack(fr["tables"]), specs, 1,
                      out, fr["info"].pixel_bytes)
    return out[:fr["want"].size]


def run_mixed(ctx, frames, device, fill=0x5A, align=256):
    """the frames' records back to back, pixel records `align` apart at least -> the pixel buffer and the offsets"""
    import torch
    co, po, c, p = [], [], 0, 0
    for fr in frames:
        co.append(c)
        po.append(p)
        c += fr["coefs"].size
        p += -(-fr["want"].size // align) * align
    coefs = np.concatenate([fr["coefs"] for fr in frames] + [np.zeros(64, np.int16)])
    pixels = np.full(p + 8, fill, dtype=np.uint8)
    infos = [fr["info"] for fr in frames]
    if device:
        d_c, d_p = torch.from_numpy(coefs).cuda(), torch.from_numpy(pixels).cuda()
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.decode_frames_mixed(d_c, co, infos, d_p, po)
        ctx.synchronize()
        ctx.reset_stream()
        pixels = d_p.cpu().numpy()
    else:
        ctx.decode_frames_mixed(coefs, co, infos, pixels, po)
    return pixels, po


def check_records(frames, pixels, po, fill=0x5A):
    end = 0
    for k, (fr, off) in enumerate(zip(frames, po)):
        assert (pixels[end:off] == fill).all(), k                    # the padding between records is nobody's to write
        assert np.array_equal(pixels[off:off + fr["want"].size], fr["want"]), k
        end = off + fr["want"].size
    assert (pixels[end:] == fill).all()


@pytest.fixture(scope="module")
def shapes():
    ql, qc = table(0, 75), table(1, 75)
    return [
        make_frame([(1, 1, 0)], [ql], 11),                                    # 8 x 8 grey: one block
        make_frame([(8, 8, 0), (4, 4, 1), (4, 4, 1)], [ql, qc], 21),          # 64 x 64 4:2:0: planes of 64 / 16 / 16 blocks
        make_frame([(9, 8, 0), (9, 8, 1), (9, 8, 1)], [ql, qc], 31),          # 72 x 64 4:4:4: 72 blocks, a unit boundary
        make_frame([(1, 257, 0)], [qc], 41),                                  # 8 x 2056 grey: bw = 1, a workgroup boundary
        make_frame([(66, 33, 0), (33, 33, 1), (33, 33, 1)], [ql, qc], 51),    # 520 x 264 4:2:2
        make_frame([(4, 3, 0), (0, 3, 1), (2, 2, 1)], [ql, qc], 61),          # a zero-size component
    ]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_records_of_different_geometry(ctx, shapes, device, reverse):
    frames = shapes[::-1] if reverse else shapes
    pixels, po = run_mixed(ctx, frames, device)
    check_records(frames, pixels, po)                                         # == the restatement
    for fr, off in zip(frames, po):                                           # == hvc_decode_frames on that frame alone
        assert np.array_equal(pixels[off:off + fr["want"].size], alone(ctx, fr))
    assert ctx.last_wide_blocks() == 0


def test_a_set_without_a_block_launches_nothing(ctx):
    fr = make_frame([(0, 3, 0), (2, 0, 0)], [table(0, 50)], 1)
    ctx.decode_frames_mixed(np.zeros(64, np.int16), [0], [fr["info"]], np.zeros(8, np.uint8), [0])
    ctx.decode_frames_mixed(np.zeros(64, np.int16), [], [], np.zeros(8, np.uint8), [])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_adjacent_frames_with_different_tables(ctx, device):
    """qualities 20, 75 and 95 side by side plus a 16-bit table (an entry of 300): a wrong table index or a lost wide flag
    changes bytes"""
    q16 = table(0, 50).copy()
    q16[5] = 300
    planes = [(7, 5, 0), (5, 3, 1)]
    frames = [make_frame(planes, [table(0, q), table(1, q)], 100 + q) for q in (20, 75, 95)]
    frames.insert(2, make_frame(planes, [q16, table(1, 20)], 300))
    frames.append(make_frame(planes, [table(0, 20), table(1, 20)], 400))      # the first tables again, other records
    pixels, po = run_mixed(ctx, frames, device)
    check_records(frames, pixels, po)
    for fr, off in zip(frames, po):
        assert np.array_equal(pixels[off:off + fr["want"].size], alone(ctx, fr))
    run_mixed(ctx, frames, device)
    assert ctx.last_wide_blocks() == 35                                       # the 16-bit table's plane, whole, and nothing else


def test_blocks_that_trip_the_int32_guard(ctx):
    """dense +-2047 coefficients at quality 1 tables leave the proven int32 range: those blocks come out in the model's 63-bit
    arithmetic, and hvc_set_decode_kernel(ctx, 2) -- every block that way -- gives the same bytes"""
    q1l, q1c = table(0, 1), table(1, 1)
    rng = np.random.Generator(np.random.PCG64(5))
    base = [synth_coefs(70 + i, bh, bw, q)[0].copy() for i, (bw, bh, q) in enumerate(((9, 8, q1l), (5, 4, q1c)))]
    for b in (0, 37, 63, 64, 71):
        base[0].reshape(-1, 64)[b] = rng.choice(np.array([-2047, 2047], dtype=np.int16), size=64)
    frames = [make_frame([(3, 3, 0)], [table(0, 75)], 7), make_frame([(9, 8, 0), (5, 4, 1)], [q1l, q1c], 0, coefs=base),
              make_frame([(2, 5, 0)], [table(1, 90)], 8)]
    for device in (False, True):
        pixels, po = run_mixed(ctx, frames, device)
        check_records(frames, pixels, po)
        wide = ctx.last_wide_blocks()
        assert 5 <= wide < 20, wide
        ctx.set_decode_kernel(2)
        try:
            again, _ = run_mixed(ctx, frames, device)
            assert ctx.last_wide_blocks() == 9 + 72 + 20 + 10
        finally:
            ctx.set_decode_kernel(0)
        assert np.array_equal(again, pixels)


# ---------------------------------------------------------------------------
# files

@pytest.fixture(scope="module")
def file_set():
    files = [golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")]
    for si in (0, 1, 3, 4, 6, 8, 9, 10, 11):
        files.append(unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 40, 24, 100 * si + 40)[0])
    for si in (2, 5, 7, 8, 10):
        files.append(unusual_sampling_file(UNUSUAL_SAMPLINGS[si], 97, 51, 100 * si + 97)[0])
    for seed in (1, 2):   # one geometry, different optimised Huffman tables (fitted to each file's own symbols)
        files.append(jpeg_optimised_tables(96, 64, 420, QT, random_record([(2, 2), (1, 1), (1, 1)], 96, 64, seed)[0]))
    models = []
    for f in files:
        d = orc.Decoder(f)
        d.decode()
        models.append([d.plane(i).copy() for i in range(d.ncomp)])
    return files, models


def check_files(results, models, skip=()):
    for f, ((status, info, planes), want) in enumerate(zip(results, models)):
        if f in skip:
            continue
        assert status == 0 and len(planes) == len(want), f
        for i, (got, w) in enumerate(zip(planes, want)):
            got = got.cpu().numpy() if hasattr(got, "cpu") else got
            assert np.array_equal(got, w), (f, i)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("threads", [1, 3])
def test_files_of_mixed_sizes_samplings_and_tables(ctx, file_set, threads, device):
    files, models = file_set
    import video_coding_amd as hvc
    coef_bytes = [2 * hvc.hvc.jpeg_read_header(f).coef_count for f in files]
    chunk = 40000                                  # Mouse480 alone is larger (its ring slot grows); the others fill several chunks
    assert max(coef_bytes) > chunk and sum(coef_bytes) - max(coef_bytes) > 3 * chunk
    results = ctx.jpeg_decode_batch_mixed(files, threads=threads, chunk_bytes=chunk, device=device)
    check_files(results, models)
    st = ctx.last_batch_stats
    assert st.chunks >= 5 and st.threads == threads and st.coef_bytes == sum(coef_bytes) and 1 <= st.frames_per_chunk < len(files)
    if threads == 1 and not device:                # == hvc_jpeg_decode of every file
        for f, (status, info, planes) in zip(files, results):
            i1, px = ctx.jpeg_decode(f)
            for a, b in zip(planes, i1.planes(px)):
                assert np.array_equal(a, b)
        one = ctx.jpeg_decode_batch_mixed(files)   # the default: everything in one chunk
        check_files(one, models)
        assert ctx.last_batch_stats.chunks == 1 and ctx.last_batch_stats.frames_per_chunk == len(files)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_failing_file_stops_nobody_else(ctx, file_set, device):
    import torch
    import video_coding_amd as hvc
    files, models = file_set
    files, models = list(files), list(models)
    info = hvc.hvc.jpeg_read_header(files[1])
    # cut in its scan.  (A scan that merely ends reads as zero bits, which the model and the reader take for valid codes: the
    # cut is followed by one-bits, which no Huffman table has a code for -- the reader fails 2000 bytes into the scan.)
    cut = files[1][:info.ecs_offset + 2000] + b"\xff\x00" * 64 + b"\xff\xd9"
    with pytest.raises(hvc.HvcError) as e:
        hvc.hvc.jpeg_entropy_decode(cut)
    cut_code = e.value.code
    garbage = np.random.Generator(np.random.PCG64(3)).integers(0, 256, size=3000, dtype=np.uint8).tobytes()
    rec = np.zeros(3 * 64 * 64, dtype=np.int64).reshape(3, 64, 64)
    rec[0, :, 0] = 2047 * (np.arange(64) + 1)                                 # absolute DCs up to 131 008: beyond int16
    q = np.stack([table(0, 75), table(1, 75)])
    wide_dc = jpeg_optimised_tables(64, 64, 444, q, rec.reshape(-1), table_sets=2)
    bad = {3: (cut, cut_code), 9: (garbage, None), 14: (wide_dc, -5)}
    for at in sorted(bad):
        files.insert(at, bad[at][0])
        models.insert(at, None)
    lay = hvc.hvc.jpeg_mixed_layout(files)
    assert lay.status[9] != 0 and lay.status[3] == 0 and lay.status[14] == 0
    pixels = np.full(lay.total_bytes, 0xA5, dtype=np.uint8)
    if device:
        pixels = torch.from_numpy(pixels).cuda()
    results = ctx.jpeg_decode_batch_mixed(files, threads=2, chunk_bytes=60000, device=device, layout=lay, pixels=pixels)   # the call itself: HVC_OK
    check_files(results, models, skip=bad)
    assert results[3][0] == cut_code != 0 and results[14][0] == -5 and results[9][0] == lay.status[9] and results[9][2] is None
    host = pixels.cpu().numpy() if device else pixels
    for at in (3, 14):                                                        # their records keep the sentinel
        off = lay.pixel_offsets[at]
        assert (host[off:off + lay.infos[at].pixel_bytes] == 0xA5).all(), at
    good_files, good_models = file_set                                        # and the context decodes another batch
    check_files(ctx.jpeg_decode_batch_mixed(good_files[:6], threads=2, device=device), good_models[:6])


# the seam between the chunk plan (csrc/hvc_mixed_decode_chunks.cpp, tests/test_mixed_decode_chunks.py) and the pipeline: six small
# files in three chunks, the third file's scan spoilt, host memory filled with a canary
SEAM_SET = [(24, 18, [(2, 2), (1, 1), (1, 1)]), (8, 8, [(1, 1)] * 3), (16, 16, [(2, 2), (1, 1), (1, 1)]), (16, 8, [(2, 1), (1, 1), (1, 1)]),
            (9, 9, [(1, 1)] * 3), (16, 16, [(2, 2), (1, 1), (1, 1)])]
SEAM_BAD, SEAM_CHUNK_BYTES, SEAM_CHUNKS, CANARY = 2, 2400, [[0], [1, 2, 3], [4, 5]], 0xA5


@pytest.fixture(scope="module")
def seam_set():
    """(files, the spoilt file's code, per form the bytes hvc_jpeg_decode / _rgb / _scaled give every good file)"""
    import video_coding_amd as hvc
    files = [jpeg_optimised_tables(w, h, s, QT, random_record(s, w, h, 7 + f)[0], table_sets=2) for f, (w, h, s) in enumerate(SEAM_SET)]
    info = hvc.hvc.jpeg_read_header(files[SEAM_BAD])
    files[SEAM_BAD] = files[SEAM_BAD][:info.ecs_offset] + b"\xff\x00" * 64 + b"\xff\xd9"   # one-bits: a code no table has
    with pytest.raises(hvc.HvcError) as e:
        hvc.hvc.jpeg_entropy_decode(files[SEAM_BAD])
    cuts, limit = [[]], SEAM_CHUNK_BYTES                                      # the cut as the header words it
    for f, data in enumerate(files):
        cb = 2 * hvc.hvc.jpeg_read_header(data).coef_count
        if cuts[-1] and sum(c for _, c in cuts[-1]) + cb > limit:
            cuts.append([])
        cuts[-1].append((f, cb))
    assert [[f for f, _ in k] for k in cuts] == SEAM_CHUNKS
    c = hvc.Context(0)
    try:
        want = {"planes": {}, "rgb": {}, "scale2": {}}
        for f, data in enumerate(files):
            if f != SEAM_BAD:
                want["planes"][f] = c.jpeg_decode(data)[1].copy()
                want["rgb"][f] = c.jpeg_decode_rgb(data)[1].copy()
                want["scale2"][f] = c.jpeg_decode_scaled(data, 2)[1].copy()
    finally:
        c.close()
    return files, e.value.code, want


@pytest.mark.parametrize("reader", ["host", "gpu"])
@pytest.mark.parametrize("form", ["planes", "rgb", "scale2"])
def test_chunks_runs_and_a_failing_file_in_host_memory(ctx, seam_set, form, reader):
    """Every good file's bytes are the single-file call's; the failing file's record, the 4096 bytes in front of it and behind it,
    the five bytes behind every RGB row and every other byte that is no good file's still hold the canary; a status per file."""
    import video_coding_amd as hvc
    h = hvc.hvc
    files, bad_code, want = seam_set
    ctx.set_mixed_reader(reader)
    lay = {"planes": lambda: h.MixedLayout(files, 8), "rgb": lambda: h.MixedRgbLayout(files, "interleaved", 0, 0),
           "scale2": lambda: h.MixedScaledLayout(files, 2)}[form]()
    assert list(lay.status) == [0] * 6
    offsets = lay.rgb_offsets if form == "rgb" else lay.pixel_offsets
    at, span = 8 if form == "planes" else 5, []                               # (full-size planes lie on 8 bytes, the others anywhere)
    for f in range(6):
        if form == "rgb":
            lay.rgb_row_strides[f] = 3 * lay.infos[f].width + 5
            span.append((lay.infos[f].height - 1) * lay.rgb_row_strides[f] + 3 * lay.infos[f].width)
        else:
            span.append((lay.infos if form == "planes" else lay.scaled)[f].pixel_bytes)
        if f in (SEAM_BAD, SEAM_BAD + 1):
            at += 4096
        offsets[f] = at
        at += span[f]
    buf = np.full(at + 64, CANARY, dtype=np.uint8)
    if form == "planes":
        res = ctx.jpeg_decode_batch_mixed(files, threads=2, chunk_bytes=SEAM_CHUNK_BYTES, layout=lay, pixels=buf)
    elif form == "rgb":
        res = ctx.jpeg_decode_batch_mixed_rgb(files, threads=2, chunk_bytes=SEAM_CHUNK_BYTES, rgb_layout=lay, rgb=buf)
    else:
        res = ctx.jpeg_decode_batch_mixed_scaled(files, 2, threads=2, chunk_bytes=SEAM_CHUNK_BYTES, layout=lay, pixels=buf)
    assert [r[0] for r in res] == [bad_code if f == SEAM_BAD else 0 for f in range(6)] and bad_code != 0
    assert ctx.last_batch_stats.chunks >= 3                                   # (the GPU reader's hand-back pass adds its own)
    theirs = np.zeros(buf.size, dtype=bool)                                   # the bytes that are a good file's
    for f in range(6):
        if f == SEAM_BAD:
            continue
        if form == "rgb":
            w, hh, rs = lay.infos[f].width, lay.infos[f].height, lay.rgb_row_strides[f]
            assert np.array_equal(h.rgb_view(buf, offsets[f], rs, w, hh, "interleaved"), want[form][f]), f
            for y in range(hh):
                theirs[offsets[f] + y * rs:offsets[f] + y * rs + 3 * w] = True
        else:
            assert np.array_equal(buf[offsets[f]:offsets[f] + span[f]], want[form][f]), f
            theirs[offsets[f]:offsets[f] + span[f]] = True
    lo, hi = offsets[SEAM_BAD], offsets[SEAM_BAD] + span[SEAM_BAD]
    assert (buf[lo - 4096:hi + 4096] == CANARY).all() and not theirs[lo - 4096:hi + 4096].any()
    assert (buf[~theirs] == CANARY).all() and theirs.sum() == sum(want[form][f].size for f in want[form])


def test_restart_markers(ctx):
    """one file with DRI, hvc_set_restart_markers on and off, against hvc_jpeg_decode under the same setting.  Off is the model's
    reading: the scan ends at the first RSTn and zero bits follow.  The first file is built so that this reading stays inside
    int16 (flat DCs, mostly empty blocks: zero bits are its shortest codes); the second is one whose reading piles DC
    differences up beyond int16, which hvc_jpeg_decode decodes through its side list and the mixed batch, which has none,
    answers with HVC_E_RANGE for that file alone."""
    import video_coding_amd as hvc
    rec, n_mcu = random_record([(2, 2), (1, 1), (1, 1)], 200, 72, 9)
    blocks = rec.reshape(-1, 64).copy()
    rng = np.random.Generator(np.random.PCG64(1))
    blocks[:, 0] = 40
    blocks[rng.integers(0, len(blocks), size=30), 0] = rng.integers(-200, 200, size=30)
    blocks[rng.random(len(blocks)) < 0.6, 1:] = 0
    tame = blocks.reshape(-1)
    marked = jpeg_optimised_tables(200, 72, 420, QT, tame, restart_interval=5)
    piling = jpeg_optimised_tables(200, 72, 420, QT, rec, restart_interval=5)
    hvc.hvc.jpeg_entropy_decode(marked)                                       # the model's reading fits the record ...
    with pytest.raises(hvc.HvcError) as e:
        hvc.hvc.jpeg_entropy_decode(piling)                                   # ... and this one's does not
    assert e.value.code == -5
    files = [golden_bytes("mini.jpg"), marked, piling]
    for honour in (False, True, False):
        ctx.set_restart_markers(honour)
        try:
            results = ctx.jpeg_decode_batch_mixed(files, threads=2)
            assert [r[0] for r in results] == [0, 0, 0 if honour else -5]
            for f, (status, info, planes) in zip(files, results):
                if status:
                    continue
                i1, px = ctx.jpeg_decode(f)                                   # the same setting, one file at a time
                for a, b in zip(planes, i1.planes(px)):
                    assert np.array_equal(a, b)
        finally:
            ctx.set_restart_markers(False)
        if honour:                                                            # == the same records written without markers
            for k, r in ((1, tame), (2, rec)):
                d = orc.Decoder(jpeg_optimised_tables(200, 72, 420, QT, r))
                d.decode()
                for i, p in enumerate(results[k][2]):
                    assert np.array_equal(p, d.plane(i))


def test_argument_checks(ctx, shapes):
    import video_coding_amd as hvc
    fr = shapes[1]
    coefs, pixels = fr["coefs"], np.full(fr["want"].size + 64, 0x11, dtype=np.uint8)
    with pytest.raises(hvc.HvcError) as e:
        ctx.decode_frames_mixed(coefs, [0], [fr["info"]], pixels, [4])        # a pixel record off 8 bytes
    assert e.value.code == -4
    with pytest.raises(hvc.HvcError) as e:
        ctx.decode_frames_mixed(coefs, [0, 4], [fr["info"]] * 2, pixels, [0, 0])   # a coefficient record off 16 bytes
    assert e.value.code == -4
    ctx.set_arithmetic("hardcaml")
    try:
        with pytest.raises(hvc.HvcError) as e:
            ctx.decode_frames_mixed(coefs, [0], [fr["info"]], pixels, [0])
        assert e.value.code == -1
        with pytest.raises(hvc.HvcError) as e:
            ctx.jpeg_decode_batch_mixed([golden_bytes("mini.jpg")])
        assert e.value.code == -1
    finally:
        ctx.set_arithmetic("model")
    assert (pixels == 0x11).all()
    ctx.decode_frames_mixed(coefs, [0], [fr["info"]], pixels, [8])
    assert np.array_equal(pixels[8:8 + fr["want"].size], fr["want"]) and (pixels[:8] == 0x11).all()


def test_profiling_brackets_the_mixed_kernel(ctx, shapes):
    import torch
    ctx.set_profiling(True)
    try:
        run_mixed(ctx, shapes, True)
        ms = ctx.last_kernel_ms()
    finally:
        ctx.set_profiling(False)
    assert 0 < ms < 50


def test_cli_decode_frames(tmp_path, capsys):
    from video_coding_amd.__main__ import main
    golden = pathlib.Path(GOLDEN)
    third = tmp_path / "third.jpg"
    third.write_bytes(jpeg_optimised_tables(96, 64, 420, QT, random_record([(2, 2), (1, 1), (1, 1)], 96, 64, 4)[0]))
    ins = [golden / "mini.jpg", golden / "Mouse480.jpg", third]
    out = tmp_path / "out"
    main(["model", "decode", "frames", str(out)] + [str(p) for p in ins])
    for p in ins:
        one = tmp_path / (p.stem + "_one.yuv")
        main(["model", "decode", "frame", str(p), str(one)])
        assert (out / (p.stem + ".yuv")).read_bytes() == one.read_bytes(), p
    broken = tmp_path / "broken.jpg"
    broken.write_bytes(golden_bytes("mini.jpg")[:100])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        main(["model", "decode", "frames", str(tmp_path / "out2"), str(ins[0]), str(broken)])
    assert e.value.code == 1 and "broken.jpg" in capsys.readouterr().err
    assert (tmp_path / "out2" / "mini.yuv").read_bytes() == (out / "mini.yuv").read_bytes()
