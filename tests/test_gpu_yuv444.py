"""hvc_decode_frames_yuv444: the block stage, Decoder.get_yuv_frame's crop (decoder.ml:403-420) and
Planar_444.convert_from_420 (tools/src/planar_444.ml:82-131) fused in one pass on the GPU, against
the CPU oracle composed the way the reference composes them:
    decode planes -> crop to actual size -> supersample_hv2 on the cropped chroma planes.
The sizes that take the kernels through every chroma tile plan (64, 128 and 256 blocks wide, one to three tiles across, the last
column in an ordinary or an overlap lane, 16-byte and byte stores) are tests/tiles444.py CASES."""
import numpy as np
import pytest

import tiles444 as t4
from helpers import synth_pixels
from oracle import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


def geometry420(width, height):
    """Decoder.init for a 4:2:0 scan (decoder.ml:304-345): planes rounded to the 16 x 16 MCU."""
    rw, rh = (width + 15) // 16 * 16, (height + 15) // 16 * 16
    return [(rw // 8, rh // 8, 0), (rw // 16, rh // 16, 1), (rw // 16, rh // 16, 1)]


def make_record(seed, planes, qtabs, adversarial=0.0):
    """One frame's coefficient record (valid blocks from the oracle's forward path; a fraction of
    blocks replaced by dense +-2047 coefficients that leave the int32 kernel's proven range)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rec = []
    for i, (bw, bh, qt) in enumerate(planes):
        c = orc.fdct_quant(synth_pixels(seed * 8 + i, bh * 8, bw * 8), qtabs[qt], bw, bh).reshape(bh * bw, 64)
        if adversarial:
            pick = rng.random(bh * bw) < adversarial
            c[pick] = rng.choice(np.array([-2047, 2047, -1024, 1023], dtype=np.int16), size=(int(pick.sum()), 64))
        rec.append(c.reshape(-1))
    return np.concatenate(rec)


def expected444(rec, planes, qtabs, width, height):
    out, off = [], 0
    for i, (bw, bh, qt) in enumerate(planes):
        n = bw * bh * 64
        plane = orc.dequant_idct_recon(rec[off:off + n], qtabs[qt], bw, bh).reshape(bh * 8, bw * 8)
        off += n
        if i == 0:
            out.append(plane[:height, :width])
        else:
            out.append(orc.supersample_hv2(np.ascontiguousarray(plane[:height // 2, :width // 2])))
    return np.concatenate([p.reshape(-1) for p in out])


def tables(quality=75):
    return np.stack([orc.quant_scale(orc.quant_luma(), quality), orc.quant_scale(orc.quant_chroma(), quality)]).astype(np.uint16)


def run(ctx, recs, planes, qtabs, width, height, device, frame_stride=None):
    import torch
    import video_coding_amd as hvc
    specs, cfs, _ = hvc.hvc.frame_layout(planes)
    n = len(recs)
    fs = frame_stride or 3 * width * height
    coefs = np.stack(recs)
    if device:
        d_c = torch.from_numpy(coefs).cuda()
        d_o = torch.full((n * fs,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.decode_frames_yuv444(d_c, cfs, qtabs, specs, n, width, height, d_o, fs)
        ctx.synchronize()
        return d_o.cpu().numpy().reshape(n, fs)
    out = np.full((n, fs), 0xA5, dtype=np.uint8)
    ctx.decode_frames_yuv444(coefs, cfs, qtabs, specs, n, width, height, out, fs)
    return out


@pytest.mark.parametrize("width,height", [
    # (what each size is to the tile plan today -- chroma tiles 64, 128 or 256 blocks wide, NW = 1, 2, 4: tests/tiles444.py
    # restates it and tests/test_tiles444.py checks these sizes too.  All of them are one tile across; the sizes with more
    # are tiles444.CASES, below.)
    (64, 48),      # NW = 1, one tile, block aligned
    (64, 40),      # chroma crop ends inside a block row (ah = 20)
    (1056, 144),   # chroma 66 blocks x 72 rows: one NW = 2 tile across, three down (seams at rows 31, 63)
    (2080, 80),    # chroma 130 blocks wide: one NW = 4 tile across, two down
    (1024, 32),    # chroma exactly 64 blocks wide: one NW = 1 tile, lane 63 (the overlap lane) owns the last column
    (1040, 32),    # 65 blocks: the first width of NW = 2, lane 64 owns the last column
    (2032, 32),    # 127 blocks: one NW = 2 tile with its overlap lane idle
    (48, 272),     # chroma 136 rows: five tiles down
    (1920, 1080),  # the headline geometry: 1088 decoded rows, crop at 1080 / 540; NW = 2, 17 tiles down
])
@pytest.mark.parametrize("device", [True, False])
def test_fused_444_equals_decode_crop_upsample(ctx, width, height, device):
    planes, qt = geometry420(width, height), tables()
    recs = [make_record(3 + f, planes, qt) for f in range(2)]
    got = run(ctx, recs, planes, qt, width, height, device)
    for f, rec in enumerate(recs):
        want = expected444(rec, planes, qt, width, height)
        assert np.array_equal(got[f], want), (f, int(np.flatnonzero(got[f] != want)[0]))
    assert ctx.last_wide_blocks() == 0


@pytest.mark.parametrize("width,height", [(52, 44), (100, 30), (18, 10), (2, 2), (1042, 70), (24, 8)])
def test_unaligned_sizes_take_the_byte_path(ctx, width, height):
    """width % 16 != 0: rows are not 16-byte aligned, the kernel stores bytes with bounds checks."""
    planes, qt = geometry420(width, height), tables(60)
    recs = [make_record(11 + f, planes, qt) for f in range(3)]
    got = run(ctx, recs, planes, qt, width, height, True)
    for f, rec in enumerate(recs):
        assert np.array_equal(got[f], expected444(rec, planes, qt, width, height)), f


def test_frame_stride_padding_is_left_untouched(ctx):
    width, height = 64, 32
    planes, qt = geometry420(width, height), tables()
    recs = [make_record(21 + f, planes, qt) for f in range(3)]
    fs = 3 * width * height + 48
    got = run(ctx, recs, planes, qt, width, height, True, frame_stride=fs)
    for f, rec in enumerate(recs):
        assert np.array_equal(got[f][:3 * width * height], expected444(rec, planes, qt, width, height))
        assert (got[f][3 * width * height:] == 0xA5).all()


@pytest.mark.parametrize("width,height", [(1056, 144), (80, 48), (52, 44)])
def test_guard_failures_go_through_the_wide_kernel_and_the_reinterpolation(ctx, width, height):
    """Blocks outside the int32 kernel's proven range: int64 kernel writes the source samples, the
    third pass rebuilds every interpolated sample that reads them (incl. the neighbours' edges)."""
    planes, qt = geometry420(width, height), tables(90)
    recs = [make_record(31 + f, planes, qt, adversarial=0.07) for f in range(2)]
    got = run(ctx, recs, planes, qt, width, height, True)
    assert ctx.last_wide_blocks() > 0
    for f, rec in enumerate(recs):
        want = expected444(rec, planes, qt, width, height)
        assert np.array_equal(got[f], want), (f, int(np.flatnonzero(got[f] != want)[0]))


def test_all_blocks_adversarial(ctx):
    width, height = 1056, 80
    planes, qt = geometry420(width, height), tables(100)
    recs = [make_record(41, planes, qt, adversarial=1.0)]
    got = run(ctx, recs, planes, qt, width, height, True)
    assert np.array_equal(got[0], expected444(recs[0], planes, qt, width, height))


def test_three_implementations_agree(ctx):
    """packed + fix-up, wide-only (int64 for every block) and 16-bit tables (wide-only by rule)."""
    width, height = 1056, 144
    planes, qt = geometry420(width, height), tables(50)
    recs = [make_record(51 + f, planes, qt, adversarial=0.02) for f in range(2)]
    a = run(ctx, recs, planes, qt, width, height, True)
    ctx.set_decode_kernel(2)
    try:
        b = run(ctx, recs, planes, qt, width, height, True)
    finally:
        ctx.set_decode_kernel(0)
    assert np.array_equal(a, b)
    for f, rec in enumerate(recs):
        assert np.array_equal(a[f], expected444(rec, planes, qt, width, height))
    qt16 = qt.copy()
    qt16[0, 63] = 300  # an entry above 255 sends the whole call to the int64 kernel
    c = run(ctx, recs[:1], planes, qt16, width, height, True)
    assert np.array_equal(c[0], expected444(recs[0], planes, qt16, width, height))


def test_equals_the_separate_kernels_at_full_size(ctx):
    """1080p x 12 frames: fused output == hvc_decode_frames -> crop -> hvc_upsample420 (product path,
    three kernels) on every frame; frame 0 also against the oracle."""
    import torch
    import video_coding_amd as hvc
    width, height = 1920, 1080
    planes, qt = geometry420(width, height), tables()
    specs, cfs, pfs = hvc.hvc.frame_layout(planes)
    base = [make_record(61 + f, planes, qt) for f in range(3)]
    n = 12
    d_c = torch.from_numpy(np.stack(base)).cuda().repeat(4, 1).contiguous()
    d_o = torch.zeros((n, 3 * width * height), dtype=torch.uint8, device="cuda")
    d_p = torch.zeros((n, pfs), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.decode_frames_yuv444(d_c, cfs, qt, specs, n, width, height, d_o)
    ctx.decode_frames(d_c, cfs, qt, specs, n, d_p, pfs)
    ctx.synchronize()
    ref = torch.zeros_like(d_o)
    ref[:, :width * height] = d_p[:, :planes[0][0] * 8 * planes[0][1] * 8].reshape(n, -1, planes[0][0] * 8)[:, :height, :width].reshape(n, -1)
    cw, ch = width // 2, height // 2
    for i in (1, 2):
        off = specs[i]["plane_offset"]
        pw, ph = planes[i][0] * 8, planes[i][1] * 8
        src = d_p[:, off:off + pw * ph].reshape(n, ph, pw)[:, :ch, :cw].contiguous()
        dst = torch.zeros((n, height, width), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.upsample420(src, cw, ch, dst, n_planes=n)
        ctx.synchronize()
        ref[:, i * width * height:(i + 1) * width * height] = dst.reshape(n, -1)
    assert torch.equal(d_o, ref)
    assert np.array_equal(d_o[0].cpu().numpy(), expected444(base[0], planes, qt, width, height))


# ---- the tile plan: tests/tiles444.py CASES (what each row pins is written there; tests/test_tiles444.py holds the rows to it) ----
_CASE_REFERENCE = {}


def case_reference(width, height):
    """two frames' records and the oracle's frames for a size, computed once and read-only"""
    if (width, height) not in _CASE_REFERENCE:
        planes, qt = geometry420(width, height), tables()
        recs = [make_record(81 + f, planes, qt) for f in range(2)]
        want = [expected444(rec, planes, qt, width, height) for rec in recs]
        for a in recs + want:
            a.setflags(write=False)
        _CASE_REFERENCE[width, height] = planes, qt, recs, want
    return _CASE_REFERENCE[width, height]


def run_case(ctx, case, recs, planes, qt, device):
    """the frames of a CASES row into a buffer of 0xA5 -> (the bytes before the first frame, [frames][frame_stride])"""
    import torch
    import video_coding_amd as hvc
    specs, cfs, _ = hvc.hvc.frame_layout(planes)
    n, fs, off = len(recs), case.frame_stride, case.offset
    coefs = np.stack(recs)
    if device:
        d_c = torch.from_numpy(coefs).cuda()
        buf = torch.full((off + n * fs,), 0xA5, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0 and (buf.data_ptr() + off) % 16 == off % 16
        torch.cuda.synchronize()
        ctx.decode_frames_yuv444(d_c, cfs, qt, specs, n, case.width, case.height, buf[off:], fs)
        ctx.synchronize()
        got = buf.cpu().numpy()
    else:
        got = np.full(off + n * fs, 0xA5, dtype=np.uint8)
        ctx.decode_frames_yuv444(coefs, cfs, qt, specs, n, case.width, case.height, got[off:], fs)
    return got[:off], got[off:].reshape(n, fs)


def check_case(case, head, got, want):
    span = 3 * case.width * case.height
    assert case.stride_extra > 0 and got.shape[1] == span + case.stride_extra
    for f in range(len(want)):
        assert np.array_equal(got[f][:span], want[f]), (f, int(np.flatnonzero(got[f][:span] != want[f])[0]))
        assert (got[f][span:] == 0xA5).all(), (f, "the bytes behind the frame")
    assert head.size == case.offset and (head == 0xA5).all(), "the bytes before the first frame"


@pytest.mark.parametrize("case", t4.CASES, ids=lambda c: c.id)
def test_tile_plan_cases_in_device_memory(ctx, case):
    planes, qt, recs, want = case_reference(case.width, case.height)
    head, got = run_case(ctx, case, recs, planes, qt, True)
    check_case(case, head, got, want)
    assert ctx.last_wide_blocks() == 0


@pytest.mark.parametrize("case", [c for c in t4.CASES if c.form == "aligned"], ids=lambda c: c.id)
def test_tile_plan_cases_with_host_buffers(ctx, case):
    planes, qt, recs, want = case_reference(case.width, case.height)
    head, got = run_case(ctx, case, recs, planes, qt, False)
    check_case(case, head, got, want)
    assert ctx.last_wide_blocks() == 0


def guard_places(g):
    """Where the placed failures go, per frame: [(plane, bx, by)].  Chroma, both planes: every shared column and the columns
    either side of it, the last column, column 0 -- each at block rows 0, 3 and 4 (either side of the first seam) where the
    crop has them, and the last block row.  Luma: one block in the first tile, the crop's last block in the last.  Frame 1
    takes every other chroma place and the second luma block alone."""
    cols = {0, g.cbw[1] - 1}
    for s in g.shared_columns():
        cols |= {s - 1, s, s + 1}
    rows = {r for r in (0, 3, 4) if r < g.cbh[1]} | {g.cbh[1] - 1}
    chroma = [(p, bx, by) for p in (1, 2) for by in sorted(rows) for bx in sorted(cols)]
    luma = [(0, min(5, g.cbw[0] - 1), 0), (0, g.cbw[0] - 1, g.cbh[0] - 1)]
    assert t4.tile_lane_of(g, *luma[0])[0] == 0 and t4.tile_lane_of(g, *luma[1])[0] == g.y_tiles - 1 > 0
    return [chroma + luma, chroma[1::2] + luma[1:]]


@pytest.mark.parametrize("width,height", [(4112, 66), (8176, 32), (8192, 80), (2030, 34)])
def test_guard_failures_at_chosen_blocks_are_each_listed_once(ctx, width, height):
    """Dense +-2047 blocks (outside the int32 guard: asserted here with the guard's restatement, as is that no other block
    of the records is) on the shared columns, beside them, in the last column and at the seams: the frames equal the
    oracle's, and the count of fix-ups equals the number of placed blocks -- a shared column's block is decoded by two
    lanes and listed by one."""
    from test_gpu_xcd_order import outside_the_model_guard
    case = [c for c in t4.CASES if (c.width, c.height) == (width, height)][0]
    g = case.geometry()
    planes, qt, base, _ = case_reference(width, height)
    places = guard_places(g)
    assert g.c_tiles_x > 1 and places[0] != places[1] and set(places[1]) < set(places[0])
    rng = np.random.Generator(np.random.PCG64(width + height))
    recs = []
    for f, rec in enumerate(base):
        blocks = rec.copy().reshape(-1, 64)
        first = 0
        for p, (bw, bh, t) in enumerate(planes):
            assert not outside_the_model_guard(blocks[first:first + bw * bh], qt[t]).any()        # the ordinary blocks stay inside
            placed = sorted(first + by * bw + bx for pp, bx, by in places[f] if pp == p)
            assert len(set(placed)) == len(placed)
            for b in placed:
                blocks[b] = rng.choice(np.array([-2047, 2047], dtype=np.int16), size=64)
            outside = first + np.flatnonzero(outside_the_model_guard(blocks[first:first + bw * bh], qt[t]))
            assert outside.tolist() == placed, (f, p)                                                   # the placed ones, all of them, leave
            first += bw * bh
        recs.append(blocks.reshape(-1))
    head, got = run_case(ctx, case, recs, planes, qt, True)
    print("%d x %d: %d + %d placed, %d fix-ups" % (width, height, len(places[0]), len(places[1]), ctx.last_wide_blocks()))
    check_case(case, head, got, [expected444(rec, planes, qt, width, height) for rec in recs])
    assert ctx.last_wide_blocks() == len(places[0]) + len(places[1])


def test_three_implementations_agree_with_the_last_column_in_an_overlap_lane(ctx):
    """test_three_implementations_agree at 8176 x 32: two NW = 4 tiles across, the last column stored by tile 1's lane 255.
    The wide-only form runs k_decode_wide_444 over every lane of every tile, and must skip the overlap lanes that do not store."""
    width, height = 8176, 32
    planes, qt = geometry420(width, height), tables(50)
    recs = [make_record(91 + f, planes, qt, adversarial=0.02) for f in range(2)]
    a = run(ctx, recs, planes, qt, width, height, True)
    ctx.set_decode_kernel(2)
    try:
        b = run(ctx, recs, planes, qt, width, height, True)
    finally:
        ctx.set_decode_kernel(0)
    assert np.array_equal(a, b)
    for f, rec in enumerate(recs):
        assert np.array_equal(a[f], expected444(rec, planes, qt, width, height))
    qt16 = qt.copy()
    qt16[0, 63] = 300
    c = run(ctx, recs[:1], planes, qt16, width, height, True)
    assert np.array_equal(c[0], expected444(recs[0], planes, qt16, width, height))


def file_444(jpg):
    """the oracle's 4:4:4 frame of a 4:2:0 file: [3][height][width]"""
    d = orc.Decoder(jpg)
    d.decode()
    y, u, v = d.get_yuv_frame()
    return np.stack([y, orc.supersample_hv2(u), orc.supersample_hv2(v)])


@pytest.mark.parametrize("width,height", [(8176, 32), (4112, 48)])
def test_wide_dc_files_across_two_tiles(ctx, width, height):
    """hvc_jpeg_decode_yuv444 on a file whose DC leaves int16 in every plane: every block goes through apply_wide_dc_444's
    inversion of the tile plan -- two NW = 4 tiles across, at 8176 the last column through the clamp of the tile index."""
    import video_coding_amd as hvc
    from test_gpu_single_file_paths import wide_dc_file
    jpg = wide_dc_file(width, height)
    info = hvc.hvc.jpeg_read_header(jpg)
    assert (info.width, info.height) == (width, height)
    g = t4.Geometry(width, height)
    assert (g.nw, g.c_tiles_x) == (4, 2)
    d = orc.Decoder(jpg)
    rec, first = np.asarray(d.coef_record()).reshape(-1, 64), 0
    for i in range(3):
        nb = d.info(i)["decoded_width"] // 8 * (d.info(i)["decoded_height"] // 8)
        assert np.abs(rec[first:first + nb, 0]).max() > 32767, i
        first += nb
    assert first == rec.shape[0]
    got = ctx.jpeg_decode_yuv444(jpg)[1]
    assert np.array_equal(got, file_444(jpg))


def telling_wide_dc_file(w, h):
    """A 4:2:0 file at quantiser 1 whose every block has a DC beyond int16 AND a sample that shows it.  The files of
    wide_dc_file cannot tell a block that apply_wide_dc_444 left out from one it rewrote: the host reader leaves such a DC
    saturated at +-32767 in the record, and with ACs of +-100 every sample of the block is 0 or 255 under either DC.  Here
    the ACs of a block are a spike against its DC at one sample (x0, y0) -- the DCT of a single sample, scaled until it
    cancels DC / 8 there, no AC beyond the baseline's +-1023 -- so that sample lands inside 0 .. 255 and moves by 29 levels
    and more between the true DC (|DC| >= 33000) and the saturated one.  The test asserts that on the CPU for every block."""
    import video_coding_amd as hvc
    from helpers import jpeg_optimised_tables
    info = hvc.hvc.jpeg_encoder_layout(w, h, 420, 100)
    rng = np.random.Generator(np.random.PCG64(7 * w + h))
    nb = info.coef_count // 64
    dc = rng.integers(33000, 40001, size=nb) * rng.choice([-1, 1], size=nb)
    x0, y0 = rng.integers(0, 8, size=nb), rng.integers(0, 8, size=nb)
    want = rng.integers(40, 216, size=nb)                        # the sample's level
    f = np.arange(8)
    cu = np.where(f == 0, np.sqrt(0.5), 1.0)
    bx, by = (cu * np.cos((2 * x0[:, None] + 1) * f * np.pi / 16)), (cu * np.cos((2 * y0[:, None] + 1) * f * np.pi / 16))
    g = 0.25 * (by[:, :, None] * bx[:, None, :]).reshape(nb, 64)  # [block][v * 8 + u]: what a coefficient adds at (x0, y0)
    g[:, 0] = 0
    target = want - 128 - dc / 8.0
    spike = lambda k: np.clip(k[:, None] * g, -1023, 1023)
    lo, hi = np.zeros(nb), np.full(nb, 1e6)
    for _ in range(50):                                          # |k|: the clipped spike's sum at (x0, y0) grows with it
        mid = (lo + hi) / 2
        reached = np.abs((spike(mid) * g).sum(axis=1)) >= np.abs(target)
        lo, hi = np.where(reached, lo, mid), np.where(reached, mid, hi)
    natural = np.rint(spike(hi * np.sign(target))).astype(np.int64)
    natural[:, 0] = dc
    rec = np.zeros((nb, 64), dtype=np.int64)
    rec[:] = natural[:, np.asarray(orc.zigzag_inverse())]        # record position k holds natural index zigzag_inverse[k]
    return jpeg_optimised_tables(w, h, 420, np.ones((2, 64), dtype=np.uint16), rec.reshape(-1))


@pytest.mark.parametrize("width,height", [(8176, 32), (4112, 48)])
def test_wide_dc_blocks_that_show_their_dc(ctx, width, height):
    """hvc_jpeg_decode_yuv444 on telling_wide_dc_file: a block that the host's inversion of the tile plan sends to a lane
    that does not store it (a shared column, the clamped last column) keeps its saturated DC and differs from the oracle."""
    jpg = telling_wide_dc_file(width, height)
    d = orc.Decoder(jpg)
    rec = np.asarray(d.coef_record()).reshape(-1, 64)
    assert np.abs(rec[:, 0]).min() >= 33000 and np.abs(rec[:, 1:]).max() <= 1023
    d.decode()
    first = 0
    for i in range(3):                                           # with the record's saturated DC every block comes out otherwise
        bw, bh = d.info(i)["decoded_width"] // 8, d.info(i)["decoded_height"] // 8
        sat = np.clip(rec[first:first + bw * bh], -32767, 32767).astype(np.int16)
        first += bw * bh
        other = orc.dequant_idct_recon(sat.reshape(-1), np.ones(64, dtype=np.uint16), bw, bh).reshape(bh, 8, bw, 8)
        differ = (other != np.asarray(d.plane(i)).reshape(bh, 8, bw, 8)).any(axis=(1, 3))
        assert differ.all(), (i, np.argwhere(~differ)[:4])
    assert first == rec.shape[0]
    got = ctx.jpeg_decode_yuv444(jpg)[1]
    assert np.array_equal(got, file_444(jpg))


def test_gpu_reader_batch_across_two_wide_tiles(ctx):
    """Three noise files of 4112 x 48 behind the GPU Huffman reader (k_decode_444 reading its compact DC plane) into device
    memory: NW = 4, two tiles across."""
    import torch
    width, height, n = 4112, 48, 3
    g = t4.Geometry(width, height)
    assert (g.nw, g.c_tiles_x, g.c_tiles_y) == (4, 2, 1)
    files = []
    for f in range(n):
        rng = np.random.Generator(np.random.PCG64(101 + f))
        y, u, v = (rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((height, width), (height // 2, width // 2), (height // 2, width // 2)))
        files.append(orc.encode_yuv(y, u, v, width, height, 420, 90))
    span = 3 * width * height
    fs = span + 64
    out = torch.full((n, fs), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = ctx.jpeg_decode_batch(files, out, fs, threads=2, frames_per_chunk=n, yuv444=True, gpu_entropy=True)
    ctx.synchronize()
    assert st.chunks == 1 and st.entropy_ms_sum == 0, "the chunk fell to the host reader"
    got = out.cpu().numpy()
    for f in range(n):
        assert np.array_equal(got[f][:span], file_444(files[f]).reshape(-1)), f
        assert (got[f][span:] == 0xA5).all(), f


def test_argument_errors(ctx):
    import video_coding_amd as hvc
    planes, qt = geometry420(64, 48), tables()
    specs, cfs, _ = hvc.hvc.frame_layout(planes)
    coefs = np.zeros(cfs, dtype=np.int16)
    out = np.zeros(3 * 64 * 48, dtype=np.uint8)
    with pytest.raises(hvc.HvcError):  # odd width: "Expecting a 4:2:0 frame" (yuv.ml:104-116)
        ctx.decode_frames_yuv444(coefs, cfs, qt, specs, 1, 63, 48, out)
    with pytest.raises(hvc.HvcError):  # crop outside the decoded planes
        ctx.decode_frames_yuv444(coefs, cfs, qt, specs, 1, 64, 66, out)
    with pytest.raises(hvc.HvcError):  # not three components
        ctx.decode_frames_yuv444(coefs, cfs, qt, specs[:2], 1, 64, 48, out)


def test_single_frame_ignores_the_frame_stride(ctx):
    import video_coding_amd as hvc
    width, height = 48, 32
    planes, qt = geometry420(width, height), tables()
    rec = make_record(71, planes, qt)
    specs, cfs, _ = hvc.hvc.frame_layout(planes)
    out = np.zeros(3 * width * height, dtype=np.uint8)
    ctx.decode_frames_yuv444(rec, cfs, qt, specs, 1, width, height, out, 16)  # host buffers, stride < frame
    assert np.array_equal(out, expected444(rec, planes, qt, width, height))


@pytest.mark.parametrize("pad", [0, 1000])
def test_host_buffers_in_four_overlapped_parts_equal_the_device_path(ctx, pad):
    """hvc_decode_frames_yuv444 with host memory, a batch above 64 MB of coefficients (uploaded, decoded and
    downloaded in four parts on two streams): same frames as the resident path, the caller's bytes between
    frames untouched."""
    import torch
    import video_coding_amd as hvc
    width, height = 1920, 1080
    planes, qt = geometry420(width, height), tables()
    specs, cfs, pfs = hvc.hvc.frame_layout(planes)
    base = [make_record(161 + f, planes, qt) for f in range(3)]
    n = 24
    batch = np.ascontiguousarray(np.stack(base)[np.arange(n) % 3])
    d_o = torch.zeros((n, 3 * width * height), dtype=torch.uint8, device="cuda")
    ctx.decode_frames_yuv444(torch.from_numpy(batch).cuda(), cfs, qt, specs, n, width, height, d_o)
    ctx.synchronize()
    want = d_o.cpu().numpy()
    fs = 3 * width * height + pad
    host = np.full((n, fs), 0x3C, dtype=np.uint8)
    ctx.decode_frames_yuv444(batch, cfs, qt, specs, n, width, height, host, frame_stride=fs)
    assert np.array_equal(host[:, :3 * width * height], want)
    assert (host[:, 3 * width * height:] == 0x3C).all()


def test_split_launch_modes_give_the_same_frames():
    """HVC_444_MODE=1 / 2 (hvc_capi.hip fused444_mode: the luma planes through k_decode_packed itself, before or beside the
    chroma tiles' kernel) are A/B alternates of the one-kernel form that ships (measured slower: profiles/r03b_ab.txt);
    the variable is read once per process, so this module runs again in child processes under both."""
    import os
    import subprocess
    import sys
    if os.environ.get("HVC_444_MODE"):
        pytest.skip("already inside a child run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for mode in ("1", "2"):
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu"], cwd=root,
                           env=dict(os.environ, HVC_444_MODE=mode), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and " passed" in r.stdout, (mode, r.stdout[-2000:], r.stderr[-2000:])
