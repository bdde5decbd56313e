"""The mixed GPU Huffman reader (csrc/hvc_hdec_mixed.hip): hvc_jpeg_entropy_decode_gpu_mixed against the host reader record by
record, and the mixed batch calls under hvc_set_mixed_reader("gpu") against the same calls under "host" -- byte for byte, no
tolerances: which reader ran never changes a result."""
import pathlib

import numpy as np
import pytest

from conftest import GOLDEN, golden_bytes
from helpers import jpeg_optimised_tables
from mixed_reader_files import flat_grey_file, reader_set, subsequences
from test_restart_intervals import QT, random_record

pytestmark = pytest.mark.gpu

ROUNDS = 22   # HVC_HDM_ROUNDS: a file of at most ROUNDS + 1 subsequences is settled whatever it holds


@pytest.fixture()
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_records():
    """the host reader's record of every file of the set, computed once"""
    import video_coding_amd as hvc
    return [hvc.hvc.jpeg_entropy_decode(f)[1] for f in reader_set()[0]]   # (raises if the host reader refuses a file)


# --- 1. records equal the host reader's

@pytest.mark.parametrize("reverse", [False, True], ids=["in-order", "reversed"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_records_equal_the_host_readers(ctx, host_records, device, reverse):
    files, names, ineligible = reader_set()
    order = list(range(len(files)))[::-1] if reverse else list(range(len(files)))
    import video_coding_amd as hvc
    # canary elements behind the last record: the reader's write passes must never store past the records
    lay = hvc.hvc.MixedLayout([files[i] for i in order], 8)
    total, guard = hvc.hvc.mixed_coef_offsets(lay)[1], 8192
    buf = np.full(total + guard, 0x5A5A, dtype=np.int16)
    if device:
        import torch
        buf = torch.from_numpy(buf).cuda()
    got = ctx.jpeg_entropy_decode_gpu_mixed(lay.jpegs, layout=lay, coefs=buf)
    tail = (buf.cpu().numpy() if device else buf)[total:]
    assert (tail == 0x5A5A).all(), "the reader wrote past the coefficient records"
    for i, (status, info, rec, used) in zip(order, got):
        assert status == 0, names[i]
        assert np.array_equal(rec, host_records[i]), names[i]
        assert used == (0 if i in ineligible else 1), names[i]
    assert len(ineligible) == 3


# --- 2. settling

def test_a_short_file_is_settled_whatever_it_holds(ctx):
    import video_coding_amd as hvc
    flat = flat_grey_file(400, 400)
    assert 2 < subsequences(flat) <= 8 <= ROUNDS + 1
    (status, info, rec, used), = ctx.jpeg_entropy_decode_gpu_mixed([flat])
    assert (status, used) == (0, 1) and np.array_equal(rec, hvc.hvc.jpeg_entropy_decode(flat)[1])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_flat_content_gives_the_right_record_whichever_reader_took_it(ctx, device):
    import video_coding_amd as hvc
    flat = flat_grey_file(512, 512)
    mini = golden_bytes("mini.jpg")
    got = ctx.jpeg_entropy_decode_gpu_mixed([mini, flat, mini], device=device)
    assert [g[0] for g in got] == [0, 0, 0]
    assert np.array_equal(got[1][2], hvc.hvc.jpeg_entropy_decode(flat)[1])
    assert np.array_equal(got[0][2], got[2][2]) and np.array_equal(got[0][2], hvc.hvc.jpeg_entropy_decode(mini)[1])


# --- 3. a failing file stops nobody else

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_failing_file_stops_nobody_else(ctx, device):
    import torch
    import video_coding_amd as hvc
    from test_gpu_mixed import check_files, table
    from oracle import orc
    files, _, _ = reader_set()
    files = list(files[:18])                                                  # the file set of tests/test_gpu_mixed.py
    models = []
    for f in files:
        d = orc.Decoder(f)
        d.decode()
        models.append([d.plane(i).copy() for i in range(d.ncomp)])
    good_files, good_models = list(files), list(models)
    info = hvc.hvc.jpeg_read_header(files[1])
    cut = files[1][:info.ecs_offset + 2000] + b"\xff\x00" * 64 + b"\xff\xd9"  # cut in its scan, one-bits behind the cut
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
    statuses = {}
    for reader in ("host", "gpu"):
        ctx.set_mixed_reader(reader)
        pixels = np.full(lay.total_bytes, 0xA5, dtype=np.uint8)
        if device:
            pixels = torch.from_numpy(pixels).cuda()
        results = ctx.jpeg_decode_batch_mixed(files, threads=2, chunk_bytes=60000, device=device, layout=lay, pixels=pixels)
        statuses[reader] = [r[0] for r in results]
        check_files(results, models, skip=bad)                                # the good files equal the model
        host = pixels.cpu().numpy() if device else pixels
        for at in (3, 14):                                                    # the failed files' records keep the sentinel
            off = lay.pixel_offsets[at]
            assert (host[off:off + lay.infos[at].pixel_bytes] == 0xA5).all(), (reader, at)
    assert statuses["gpu"] == statuses["host"]
    assert statuses["gpu"][3] == cut_code != 0 and statuses["gpu"][14] == -5 and statuses["gpu"][9] == lay.status[9] != 0
    gpu, host_n = ctx.last_mixed_reader_files()
    assert gpu > 0 and host_n >= 2 and gpu + host_n == len(files) - 1          # (the garbage file reached no reader)
    check_files(ctx.jpeg_decode_batch_mixed(good_files[:6], threads=2, device=device), good_models[:6])   # a further batch, same context


# --- 4. every form

CHUNK = 40000


def run_form(ctx, form, files, threads, reader):
    """one call of the form into a sentinel-filled host buffer -> (buffer, statuses, stats, split, layout statuses, record mask)"""
    import video_coding_amd as hvc
    h = hvc.hvc
    ctx.set_mixed_reader(reader)
    kind = form[0]
    if kind == "planes":
        lay = h.MixedLayout(files, 8)          # records of whole blocks on 8 bytes: they touch, the buffer has no byte that is nobody's
        buf = np.full(max(lay.total_bytes, 8), 0xA5, dtype=np.uint8)
        res = ctx.jpeg_decode_batch_mixed(files, threads=threads, chunk_bytes=CHUNK, layout=lay, pixels=buf)
    elif kind == "rgb":
        lay = h.MixedRgbLayout(files, "interleaved", 0, form[1])
        buf = np.full(max(lay.total_bytes, 8), 0xA5, dtype=np.uint8)
        res = ctx.jpeg_decode_batch_mixed_rgb(files, threads=threads, chunk_bytes=CHUNK, rgb_layout=lay, rgb=buf)
    elif kind == "scaled":
        lay = h.MixedScaledLayout(files, form[1])
        buf = np.full(max(lay.total_bytes, 8), 0xA5, dtype=np.uint8)
        res = ctx.jpeg_decode_batch_mixed_scaled(files, form[1], threads=threads, chunk_bytes=CHUNK, layout=lay, pixels=buf)
    else:
        lay = h.MixedScaledRgbLayout(files, form[1], "interleaved", 0, 0)
        buf = np.full(max(lay.total_bytes, 8), 0xA5, dtype=np.uint8)
        res = ctx.jpeg_decode_batch_mixed_scaled_rgb(files, form[1], threads=threads, chunk_bytes=CHUNK, rgb_layout=lay, rgb=buf)
    mask = None
    if kind == "rgb":
        # The alignment padding BETWEEN the images of a full-size host call is nobody's: include/hvc_jpeg.h lets a call overwrite it
        # (consecutive good records come home in one copy, with whatever the device slot held between them), so it is no result
        # and not compared.  Everything from an image's first byte to its last -- the bytes between its rows included -- is.
        # `nobody`: the bytes that are neither an image's nor inside the padding between two images that follow one another
        # (the only bytes such a copy can reach: a run of records ends where 4096 bytes or more lie between two of them, and at a
        # failed file); they keep the sentinel under both readers.
        mask, reach, prev_end = np.zeros(buf.size, dtype=bool), np.zeros(buf.size, dtype=bool), None
        for f in range(len(files)):
            if lay.status[f] == 0:
                w, hh = lay.infos[f].width, lay.infos[f].height
                if w > 0 and hh > 0:
                    lo, hi = lay.rgb_offsets[f], lay.rgb_offsets[f] + (hh - 1) * lay.rgb_row_strides[f] + 3 * w
                    mask[lo:hi] = True
                    if prev_end is not None and 0 <= lo - prev_end < 4096:
                        reach[prev_end:lo] = True
                    prev_end = hi
        mask = (mask, ~(mask | reach))
    return buf, [r[0] for r in res], ctx.last_batch_stats, ctx.last_mixed_reader_files(), list(lay.status), mask


FORMS = [("planes",), ("rgb", 1), ("rgb", 8), ("scaled", 2), ("scaled", 4), ("scaled", 8), ("scaled_rgb", 8)]


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("form", FORMS, ids=["-".join(map(str, f)) for f in FORMS])
def test_every_form_is_the_host_readers_byte_for_byte(ctx, form, threads):
    files = reader_set()[0]
    want, want_st, stats, (g0, h0), lay_st, mask = run_form(ctx, form, files, threads, "host")
    assert stats.chunks >= 5
    reached = sum(1 for a in lay_st if a == 0)             # (an RGB layout has already refused the samplings without an RGB image)
    assert (g0, h0) == (0, reached)
    got, got_st, stats, (g1, h1), _, _ = run_form(ctx, form, files, threads, "gpu")
    assert got_st == want_st
    if mask is None:
        assert np.array_equal(got, want)                   # the whole buffer
    else:
        mask, nobody = mask
        assert mask.sum() > 0.9 * mask.size and np.array_equal(got[mask], want[mask])
        assert (got[nobody] == 0xA5).all() and (want[nobody] == 0xA5).all()   # no stray write where no copy may reach
    assert g1 > 0 and g1 + h1 == reached
    assert stats.chunks >= 5


# --- 5. restart markers

def test_restart_markers_send_the_file_to_the_host_reader(ctx):
    rec, _ = random_record([(2, 2), (1, 1), (1, 1)], 200, 72, 9)
    marked = jpeg_optimised_tables(200, 72, 420, QT, rec, restart_interval=5)
    plain = jpeg_optimised_tables(200, 72, 420, QT, rec)
    files = [golden_bytes("mini.jpg"), marked, plain, golden_bytes("Mouse480.jpg")]
    ctx.set_restart_markers(True)
    try:
        want, want_st, _, _, _, _ = run_form(ctx, ("planes",), files, 2, "host")
        got, got_st, _, (g, h), _, _ = run_form(ctx, ("planes",), files, 2, "gpu")
    finally:
        ctx.set_restart_markers(False)
    assert got_st == want_st == [0, 0, 0, 0] and np.array_equal(got, want)
    assert (g, h) == (3, 1)                                                   # the DRI file is the host reader's


# --- 6. the default

def test_the_default_is_the_host_reader(ctx):
    assert ctx.get_mixed_reader() == "host"
    ctx.jpeg_decode_batch_mixed([golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")], threads=2)
    assert ctx.last_mixed_reader_files() == (0, 2)
    ctx.set_mixed_reader("gpu")
    assert ctx.get_mixed_reader() == "gpu"
    ctx.jpeg_decode_batch_mixed([golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")], threads=2)
    assert ctx.last_mixed_reader_files() == (2, 0)
    ctx.set_mixed_reader("host")
    assert ctx.get_mixed_reader() == "host"
    import video_coding_amd as hvc
    with pytest.raises(hvc.HvcError) as e:
        ctx.set_mixed_reader(7)
    assert e.value.code == -1


# --- 7. CLI

def test_cli_reader_gpu_writes_the_same_files(tmp_path):
    from video_coding_amd.__main__ import main
    golden = pathlib.Path(GOLDEN)
    third = tmp_path / "third.jpg"
    third.write_bytes(jpeg_optimised_tables(96, 64, 420, QT, random_record([(2, 2), (1, 1), (1, 1)], 96, 64, 4)[0]))
    ins = [str(golden / "mini.jpg"), str(golden / "Mouse480.jpg"), str(third)]
    for extra in ([], ["-rgb"], ["-scale", "4"]):
        a, b, c = tmp_path / ("a" + "".join(extra)), tmp_path / ("b" + "".join(extra)), tmp_path / ("c" + "".join(extra))
        main(["model", "decode", "frames", str(a)] + ins + extra)
        main(["model", "decode", "frames", str(b)] + ins + extra + ["-reader", "gpu"])
        main(["model", "decode", "frames", str(c)] + ins + extra + ["-reader", "host"])
        names = sorted(p.name for p in a.iterdir())
        assert len(names) == 3 and names == sorted(p.name for p in b.iterdir()) == sorted(p.name for p in c.iterdir())
        for n in names:
            assert (a / n).read_bytes() == (b / n).read_bytes() == (c / n).read_bytes(), (extra, n)
