"""hvc_set_encode_libjpeg on the GPU (include/hvc_jpeg.h, "Encoding bit-exact to libjpeg"; csrc/hvc_libjpeg_encode.hip):
k_fdct_islow, k_dummy_blocks, k_rgb_to_ycc_libjpeg and their mixed twins through the C ABI against the numpy definition (tools/libjpeg_encode_reference.py, which
tests/test_libjpeg_encode_reference.py holds to libjpeg-turbo with 0 mismatches) and against the stored hashes of Pillow's
own records (tests/golden/libjpeg_encode_pins.json).  Every comparison is exact equality; buffers are prefilled and compared
whole, so what lies between planes and frames must keep its fill."""
import io
import json

import numpy as np
import pytest

import libjpeg_encode_cases as lc

ler = lc.ler
pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL16 = np.array([FILL, FILL], dtype=np.uint8).view(np.int16)[0]
E_INVALID_ARG = -1
# the cases hvc_jpeg_encode can state: three components, the tables of a quality (q100 is all ones)
FILE_CASES = [c for c in lc.plane_cases() if c[3] != 400 and c[5] not in ("ones", "max")]


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture(scope="module")
def ctx(hvc):
    c = hvc.Context(0)
    c.set_encode_libjpeg(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain(hvc):
    """a context that never touches the setting"""
    c = hvc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pins():
    with open(lc.PINS) as f:
        return json.load(f)


def refused(hvc, fn, *a, **k):
    with pytest.raises(hvc.hvc.HvcError) as e:
        fn(*a, **k)
    return e.value.code


# ---- the setting ----------------------------------------------------------------------------------------------------
def test_the_setting_reads_back_and_stands_alone(hvc, plain):
    c = hvc.Context(0)
    try:
        assert c.encode_libjpeg is False
        c.set_encode_libjpeg(True)
        assert c.encode_libjpeg is True and plain.encode_libjpeg is False   # (a second context is unaffected)
        for bad in (2, -1):
            assert refused(hvc, c.set_encode_libjpeg, bad) == E_INVALID_ARG and c.encode_libjpeg is True
        # independent of the other settings, either way round
        assert c.encode_arithmetic == "model" and c.arithmetic == "model" and c.mixed_arithmetic == "model"
        c.set_encode_arithmetic("hardcaml")
        c.set_arithmetic("libjpeg")
        c.set_mixed_arithmetic("libjpeg")
        assert c.encode_libjpeg is True
        c.set_encode_libjpeg(False)
        assert c.encode_libjpeg is False
        assert c.encode_arithmetic == "hardcaml" and c.arithmetic == "libjpeg" and c.mixed_arithmetic == "libjpeg"
    finally:
        c.close()


# ---- the block stage on records ---------------------------------------------------------------------------------------
PLANES = [(20, 14, 0), (5, 3, 1), (3, 2, 1)]   # 280 blocks: two workgroups and a ragged last wave; small planes beside it


def place(planes, layout):
    """specs of the planes, the int16 elements and the bytes from frame to frame; "spread": gaps everywhere"""
    spread = layout == "spread"
    specs, co, po = [], (64 if spread else 0), (16 if spread else 0)
    for bw, bh, qt in planes:
        stride = bw * 8 + (8 if spread else 0)
        specs.append(dict(blocks_w=bw, blocks_h=bh, qtab=qt, coef_offset=co, plane_offset=po, stride=stride))
        co += bw * bh * 64 + (128 if spread else 0)
        po += stride * bh * 8 + (24 if spread else 0)
    return specs, co + (64 if spread else 0), po + (40 if spread else 0)


def block_content(seed, n):
    """n blocks [n, 8, 8]: all 0, all 255, the checkerboard of 0 / 255 (the largest AC) both ways, noise, in turn"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:8, 0:8]
    kinds = [np.zeros((8, 8)), np.full((8, 8), 255), 255 * ((xx + yy) & 1), 255 * ((xx + yy + 1) & 1), None, None, None]
    return np.stack([rng.integers(0, 256, size=(8, 8)) if kinds[i % 7] is None else kinds[i % 7] for i in range(n)]).astype(np.uint8)


@pytest.fixture(scope="module")
def block_frames():
    """3 frames of PLANES: per frame and plane its samples [bh * 8, bw * 8] -- made once, never changed"""
    out = []
    for f in range(3):
        planes = []
        for i, (bw, bh, _) in enumerate(PLANES):
            b = block_content(500 + 10 * f + i, bw * bh).reshape(bh, bw, 8, 8)
            planes.append(np.ascontiguousarray(b.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)))
        out.append(planes)
    return out


@pytest.fixture(scope="module")
def block_records(block_frames):
    """{table name: per frame and plane the definition's [bh * bw, 64]}"""
    return {t: [[ler.fdct_quant_plane(p, lc.tables(t)[qt]) for p, (_, _, qt) in zip(planes, PLANES)] for planes in block_frames]
            for t in lc.TABLES}


def buffers(block_frames, records, layout, n):
    specs, cfs, pfs = place(PLANES, layout)
    px = np.full((n, pfs), FILL, dtype=np.uint8)
    want = np.full((n, cfs), FILL16, dtype=np.int16)
    for f in range(n):
        for s, p, r in zip(specs, block_frames[f], records[f]):
            for y in range(p.shape[0]):
                px[f, s["plane_offset"] + y * s["stride"]:s["plane_offset"] + y * s["stride"] + p.shape[1]] = p[y]
            want[f, s["coef_offset"]:s["coef_offset"] + r.size] = r.reshape(-1)
    return specs, cfs, pfs, px, want


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("layout", ["tight", "spread"])
@pytest.mark.parametrize("n", [1, 3])
def test_encode_frames_equals_the_definition(ctx, block_frames, block_records, where, layout, n):
    import torch
    for t in lc.TABLES:
        specs, cfs, pfs, px, want = buffers(block_frames, block_records[t], layout, n)
        got = np.full((n, cfs), FILL16, dtype=np.int16)
        if where == "host":
            ctx.encode_frames(px, pfs, lc.tables(t), specs, n, got, cfs)
        else:
            d_p, d_c = torch.from_numpy(px).cuda(), torch.from_numpy(got).cuda()
            ctx.encode_frames(d_p, pfs, lc.tables(t), specs, n, d_c, cfs)
            ctx.synchronize()
            got = d_c.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, "table %s: %d elements differ, first at frame %d element %d" % (t, len(bad), bad[0][0], bad[0][1])


@pytest.mark.parametrize("where", ["host", "device"])
def test_fdct_quant_equals_the_definition(ctx, block_frames, block_records, where):
    import torch
    bw, bh, _ = PLANES[0]
    planes = np.stack([block_frames[f][0] for f in range(3)])
    for t in lc.TABLES:
        want = np.stack([ler.fdct_quant_plane(planes[f], lc.tables(t)[1]).reshape(-1) for f in range(3)])
        got = np.full((3, bw * bh * 64 + 64), FILL16, dtype=np.int16)   # (the planes' records 64 elements apart)
        if where == "host":
            ctx.fdct_quant(planes, lc.tables(t)[1], bw, bh, 3, got, coef_plane_stride=got.shape[1])
        else:
            d_p, d_c = torch.from_numpy(planes).cuda(), torch.from_numpy(got).cuda()
            ctx.fdct_quant(d_p, lc.tables(t)[1], bw, bh, 3, d_c, coef_plane_stride=got.shape[1])
            ctx.synchronize()
            got = d_c.cpu().numpy()
        assert np.array_equal(got[:, :-64], want) and (got[:, -64:] == FILL16).all()


def test_encode_frames_submit_equals_the_definition(ctx, block_frames, block_records):
    specs, cfs, pfs, px, want = buffers(block_frames, block_records["q75"], "tight", 3)
    pin_p, pin_c = ctx.host_alloc(px.shape, np.uint8), ctx.host_alloc(want.shape, np.int16)
    pin_p[:] = px
    pin_c[:] = FILL16
    ctx.encode_frames_submit(1, pin_p, pfs, lc.tables("q75"), specs, 3, pin_c, cfs)
    ctx.wait(1)
    assert np.array_equal(pin_c, want)
    ctx.host_free(pin_p)
    ctx.host_free(pin_c)


# ---- files ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def file_references():
    return {c[0]: lc.reference_record(c) for c in FILE_CASES}


def quality_of(tab):
    return 100 if tab == "ones" else int(tab[1:])   # (hvc_quant_table(100) is all ones)


@pytest.mark.parametrize("case", FILE_CASES, ids=[c[0] for c in FILE_CASES])
def test_jpeg_encode_writes_libjpegs_coefficients(ctx, pins, file_references, case):
    name, w, h, s, kind, tab = case
    y, u, v = lc.component_planes(w, h, s, kind)
    data = ctx.jpeg_encode(y, u, v, w, h, s, quality_of(tab))
    info, got = lc.file_record(data, tab)
    assert (info.width, info.height) == (w, h)
    # the file's own sampling factors: a 4:2:2 file of this library is the model's 2x2 / 1x2 / 1x2, libjpeg's (and the pins')
    # is 2x1 / 1x1 / 1x1 -- the same record where the height is a whole number of 16-row MCUs, a dummy row more elsewhere
    factors = [(info.comp[k].hscale, info.comp[k].vscale) for k in range(3)]
    same = [g[:2] for g in ler.geometry(w, h, s, factors)] == [g[:2] for g in ler.geometry(w, h, s)]
    want = file_references[name] if same else ler.encode_planes([y, u, v], w, h, s, lc.tables(tab), factors=factors)
    assert np.array_equal(got, want)
    if same:
        assert lc.sha256(got.astype("<i2")) == pins[name]   # Pillow's own record
    if lc.have_pillow():
        from PIL import Image
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (w, h)


@pytest.mark.parametrize("gpu_entropy", [False, True], ids=["host_coder", "gpu_coder"])
def test_batch_equals_the_single_file_call(ctx, gpu_entropy):
    w, h, s = 24, 24, 420
    frames, singles = [], []
    for f in range(5):
        y, u, v = [np.ascontiguousarray(p) for p in lc.content("noise", w, h, 7000 + f)]
        u, v = u[:h // 2, :w // 2].copy(), v[:h // 2, :w // 2].copy()
        frames.append(np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]))
        singles.append(ctx.jpeg_encode(y, u, v, w, h, s, 75))
    files, _ = ctx.jpeg_encode_batch(frames, w, h, s, 75, threads=2, frames_per_chunk=2, gpu_entropy=gpu_entropy)
    assert files == singles
    # and they are libjpeg's: the dummy column, the dummy row and the corner of 24 x 24 under 4:2:0
    planes = [frames[3][:w * h].reshape(h, w), frames[3][w * h:w * h + 144].reshape(12, 12), frames[3][w * h + 144:].reshape(12, 12)]
    assert np.array_equal(lc.file_record(files[3], "q75")[1], ler.encode_planes(planes, w, h, s, lc.tables("q75")))


@pytest.mark.parametrize("option", ["optimised", "restart"])
def test_the_coders_options_do_not_change_the_coefficients(hvc, file_references, option):
    case = next(c for c in FILE_CASES if c[0] == "planes_40x24_420_noise_q75")
    c = hvc.Context(0)
    try:
        c.set_encode_libjpeg(True)
        if option == "optimised":
            c.set_huffman_tables("optimised")
        else:
            c.set_restart_interval(2)
        data = c.jpeg_encode(*lc.component_planes(40, 24, 420, "noise"), 40, 24, 420, 75)
    finally:
        c.close()
    _, got = hvc.hvc.jpeg_entropy_decode(data, restart_markers=option == "restart")
    assert np.array_equal(got, file_references[case[0]])


# ---- what is refused, and the setting at 0 -----------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched_and_the_next_call_works(hvc, block_frames, block_records):
    specs, cfs, pfs, px, want = buffers(block_frames, block_records["q75"], "tight", 1)
    q = lc.tables("q75")
    c = hvc.Context(0)
    try:
        c.set_encode_libjpeg(True)
        got = np.full((1, cfs), FILL16, dtype=np.int16)
        recon = np.full((1, pfs), FILL, dtype=np.uint8)
        assert refused(hvc, c.encode_frames_recon, px, pfs, q, specs, 1, got, cfs, recon=recon) == E_INVALID_ARG
        assert (got == FILL16).all() and (recon == FILL).all()
        diff = np.full((1, sum(bw * bh for bw, bh, _ in PLANES)), FILL, dtype=np.uint8)
        assert refused(hvc, c.encode_divergence, px, pfs, q, specs, 1, max_diff=diff) == E_INVALID_ARG
        assert (diff == FILL).all()
        c.set_encode_arithmetic("hardcaml")   # the RTL's arithmetic together with the setting
        assert refused(hvc, c.encode_frames, px, pfs, q, specs, 1, got, cfs) == E_INVALID_ARG
        assert (got == FILL16).all()
        planes = lc.component_planes(16, 16, 420, "noise")
        assert refused(hvc, c.jpeg_encode, *planes, 16, 16, 420, 75) == E_INVALID_ARG
        c.set_encode_arithmetic("model")
        c.encode_frames(px, pfs, q, specs, 1, got, cfs)
        assert np.array_equal(got, want)
        frame = np.concatenate([p.reshape(-1) for p in planes])
        c.set_encode_arithmetic("hardcaml")   # (the mixed calls refuse the RTL's arithmetic as before, the setting or not)
        assert refused(hvc, c.jpeg_encode_batch_mixed, [frame], [(16, 16, 420, 75)]) == E_INVALID_ARG
        c.set_encode_arithmetic("model")
        assert c.jpeg_encode_batch_mixed([frame], [(16, 16, 420, 75)])[0][1] == c.jpeg_encode(*planes, 16, 16, 420, 75)
        assert c.jpeg_encode(*planes, 16, 16, 420, 75)[:2] == b"\xff\xd8"
    finally:
        c.close()


def test_at_0_every_file_is_what_it_was(hvc, plain):
    """a context whose setting went to 1 and back writes the bytes of one that never touched it"""
    c = hvc.Context(0)
    try:
        c.set_encode_libjpeg(True)
        c.set_encode_libjpeg(False)
        for w, h, s in [(40, 24, 420), (17, 9, 444), (24, 16, 422)]:
            planes = lc.component_planes(w, h, s, "photo")
            assert c.jpeg_encode(*planes, w, h, s, 75) == plain.jpeg_encode(*planes, w, h, s, 75)
        rgb = lc.rgb_image(40, 24, 420, "photo")
        assert c.jpeg_encode_rgb(rgb, 420, 75) == plain.jpeg_encode_rgb(rgb, 420, 75)
        frame = np.concatenate([p.reshape(-1) for p in lc.component_planes(24, 24, 420, "noise")])
        assert c.jpeg_encode_batch([frame] * 3, 24, 24, 420, 75, frames_per_chunk=2)[0] == \
            plain.jpeg_encode_batch([frame] * 3, 24, 24, 420, 75, frames_per_chunk=2)[0]
        assert c.jpeg_encode_batch_mixed([frame], [(24, 24, 420, 75)])[0][1] == plain.jpeg_encode_batch_mixed([frame], [(24, 24, 420, 75)])[0][1]
    finally:
        c.close()


def test_the_setting_changes_the_file(ctx, plain):
    """(and so every test above that passes shows something: the model's coefficients are not libjpeg's)"""
    planes = lc.component_planes(40, 24, 420, "photo")
    assert ctx.jpeg_encode(*planes, 40, 24, 420, 75) != plain.jpeg_encode(*planes, 40, 24, 420, 75)


# ---- the mixed calls: k_fdct_islow_mixed and k_dummy_blocks_mixed ----------------------------------------------------------
# every geometry of the grid at once, and in the middle a frame the encoder refuses (4:2:0 at width 16 k + 1)
MIXED_CASES = [c for c in FILE_CASES if c[4] == "noise" and c[5] == "q75"]
BAD_AT = len(MIXED_CASES) // 2


@pytest.fixture(scope="module")
def mixed_set(ctx):
    """(specs, frames, the file hvc_jpeg_encode writes for each frame alone under the setting; None for the bad one)"""
    specs, frames, alone = [], [], []
    for k, (name, w, h, s, kind, tab) in enumerate(MIXED_CASES):
        if k == BAD_AT:
            specs.append((17, 16, 420, 75))
            frames.append(np.zeros(17 * 16 * 2, dtype=np.uint8))
            alone.append(None)
        planes = lc.component_planes(w, h, s, kind)
        specs.append((w, h, s, quality_of(tab)))
        frames.append(np.concatenate([p.reshape(-1) for p in planes]))
        alone.append(ctx.jpeg_encode(*planes, w, h, s, quality_of(tab)))
    return specs, frames, alone


@pytest.mark.parametrize("coder", ["host", "gpu"])
@pytest.mark.parametrize("chunk_bytes", [0, 4096], ids=["one_chunk", "small_chunks"])
def test_mixed_batch_equals_the_single_file_call(ctx, mixed_set, coder, chunk_bytes):
    specs, frames, alone = mixed_set
    res = ctx.jpeg_encode_batch_mixed(frames, specs, threads=2, chunk_bytes=chunk_bytes, coder=coder)
    assert [r[0] for r in res] == [0 if a is not None else E_INVALID_ARG for a in alone]   # statuses as before
    assert [r[1] for r in res] == alone


@pytest.mark.parametrize("coder,option", [("host", "optimised"), ("gpu", "restart")])
def test_mixed_batch_with_the_coders_options(hvc, mixed_set, coder, option):
    specs, frames, _ = mixed_set
    c = hvc.Context(0)
    try:
        c.set_encode_libjpeg(True)
        if option == "optimised":
            c.set_huffman_tables("optimised")
        else:
            c.set_restart_interval(2)
        res = c.jpeg_encode_batch_mixed(frames, specs, threads=2, coder=coder)
        for k, (spec, fr, r) in enumerate(zip(specs, frames, res)):
            if k == BAD_AT:
                assert r[0] == E_INVALID_ARG
                continue
            w, h, s, q = spec
            info = hvc.hvc.jpeg_encoder_layout(w, h, s, q)
            sizes = [(info.comp[i].actual_width, info.comp[i].actual_height) for i in range(3)]
            assert r[0] == 0 and r[1] == c.jpeg_encode(fr[:sizes[0][0] * sizes[0][1]], fr[sizes[0][0] * sizes[0][1]:][:sizes[1][0] * sizes[1][1]],
                                                       fr[sizes[0][0] * sizes[0][1] + sizes[1][0] * sizes[1][1]:], w, h, s, q)
    finally:
        c.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_encode_frames_mixed_equals_the_definition(hvc, ctx, where):
    """records of mixed geometry: the caller's padded pixel records (replicated here), dummy blocks from the infos' sizes"""
    import torch
    cases = [c for c in MIXED_CASES]
    lay = hvc.hvc.jpeg_encoder_mixed_layout([(w, h, s, quality_of(tab)) for _, w, h, s, _, tab in cases])
    assert not any(lay.status)
    px = np.full(lay.pixel_total, FILL, dtype=np.uint8)
    want = np.full(lay.coef_total, FILL16, dtype=np.int16)
    for f, (name, w, h, s, kind, tab) in enumerate(cases):
        info = lay.infos[f]
        factors = [(info.comp[k].hscale, info.comp[k].vscale) for k in range(3)]
        planes = lc.component_planes(w, h, s, kind)
        for k, p in enumerate(planes):
            L = info.layout[k]
            rep = ler.replicate(p, L.blocks_w * 8, L.blocks_h * 8)
            at = lay.pixel_offsets[f] + L.plane_offset
            for y in range(rep.shape[0]):
                px[at + y * L.stride:at + y * L.stride + rep.shape[1]] = rep[y]
        rec = ler.encode_planes(planes, w, h, s, lc.tables(tab), factors=factors)
        want[lay.coef_offsets[f]:lay.coef_offsets[f] + rec.size] = rec
    got = np.full(lay.coef_total, FILL16, dtype=np.int16)
    if where == "host":
        ctx.encode_frames_mixed(px, lay.pixel_offsets, lay.infos, got, lay.coef_offsets)
    else:
        d_p, d_c = torch.from_numpy(px).cuda(), torch.from_numpy(got).cuda()
        ctx.encode_frames_mixed(d_p, lay.pixel_offsets, lay.infos, d_c, lay.coef_offsets)
        ctx.synchronize()
        got = d_c.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d elements differ, first at %d" % (bad.size, bad[0])


@pytest.mark.parametrize("name", ["ON", "OFF"])
def test_encode_frames_mixed_at_the_counts_where_the_workgroup_order_changes(hvc, ctx, name):
    """tests/test_gpu_mixed_counts.py's sets for the encode kernel (65535 groups: the last permuted launch; 65537: the first
    plain one), its placement and its infos, under the setting: against the numpy definition.  The infos are hand-made and
    state no size: every block is real."""
    import mixed_counts as mc
    import test_gpu_mixed_counts as tmc
    import xcd_grids as xg
    T, D, PAD, GAP = tmc.T, tmc.D, tmc.PAD, tmc.GAP

    def lje(p, q, bw, bh, stride):
        return ler.fdct_quant_plane(np.asarray(p).reshape(bh * 8, stride)[:, :bw * 8], q).reshape(-1)

    s = mc.count_set(name, zero=False)
    tabs = tmc.special_tables(s, tmc.table_pair)
    row = 8 + PAD
    P = np.stack([tmc.pixel_rows(9700 + t, 8 * D, row).reshape(D, 8 * row) for t in range(T)])
    W = np.stack([lje(P[t], tmc.table_pair(t)[0], 1, D, row).reshape(D, 64) for t in range(T)])
    pix, want = {}, {}
    for f in s.special:
        planes = s.planes(f)
        parts = [tmc.pixel_rows(9800 + 7 * f % 1000 + i, 8 * bh, 8 * bw + PAD).reshape(-1) for i, (bw, bh, _) in enumerate(planes)]
        pix[f] = np.concatenate(parts)
        want[f] = np.concatenate([lje(p, tabs[f][t], bw, bh, 8 * bw + PAD) for p, (bw, bh, t) in zip(parts, planes)])
    po, pend = mc.place(s, 8 * row, lambda f: pix[f].size, align=64)
    co, cend = mc.place(s, 64 + GAP, lambda f: want[f].size + GAP, align=8)
    pixels = np.zeros(pend + 64, dtype=np.uint8)
    mc.fill(s, pixels, po, 8 * row, lambda f: P[f % T, f % D], lambda f: pix[f])
    expect = np.full(cend + tmc.GUARD, FILL16, dtype=np.int16)
    mc.fill(s, expect, co, 64 + GAP, lambda f: W[f % T, f % D], lambda f: want[f])
    infos = mc.descriptors(hvc.hvc.JpegInfo, s, [tmc.make_info(hvc, xg.MIXED_SHAPES["grey1"], tmc.table_pair(t), pad=PAD) for t in range(T)],
                           lambda f: tmc.make_info(hvc, s.planes(f), tabs[f], pad=PAD))
    d_p, d_c = tmc.to_device(pixels, np.full(expect.size, FILL16, dtype=np.int16))
    ctx.encode_frames_mixed(d_p, mc.size_array(po), infos, d_c, mc.size_array(co))
    ctx.synchronize()
    got = d_c.cpu().numpy()
    assert np.array_equal(got, expect), tmc.first_difference(s, got, expect, co)


# ---- from RGB: k_rgb_to_ycc_libjpeg and its mixed twin -------------------------------------------------------------------------
RGB_CASES = lc.rgb_cases()


def rgb_reference(hvc, case):
    """the definition's record of an RGB case under THIS library's sampling factors (4:2:2: the model's), and whether the
    layout is Pillow's too (then the pins hold)"""
    name, w, h, s, kind, tab = case
    info = hvc.hvc.jpeg_encoder_layout(w, h, s, quality_of(tab))
    factors = [(info.comp[k].hscale, info.comp[k].vscale) for k in range(3)]
    same = [g[:2] for g in ler.geometry(w, h, s, factors)] == [g[:2] for g in ler.geometry(w, h, s)]
    return ler.encode_planes(ler.rgb_to_planes(lc.rgb_image(w, h, s, kind), s), w, h, s, lc.tables(tab), factors=factors), same


@pytest.mark.parametrize("case", RGB_CASES, ids=[c[0] for c in RGB_CASES])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_jpeg_encode_rgb_writes_libjpegs_coefficients(hvc, ctx, pins, case, layout):
    name, w, h, s, kind, tab = case
    rgb = lc.rgb_image(w, h, s, kind)
    data = ctx.jpeg_encode_rgb(rgb if layout == "interleaved" else np.ascontiguousarray(rgb.transpose(2, 0, 1)), s, quality_of(tab), layout=layout)
    info, got = lc.file_record(data, tab)
    want, same = rgb_reference(hvc, case)
    assert (info.width, info.height) == (w, h) and np.array_equal(got, want)
    if same:
        assert lc.sha256(got.astype("<i2")) == pins[name]   # Pillow's own record of this RGB image
    if lc.have_pillow():
        from PIL import Image
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (w, h)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("layout", ["interleaved", "planar"])
def test_rgb_to_yuv_makes_libjpegs_planes_and_nothing_else(hvc, ctx, where, layout):
    """the frame's own samples, libjpeg's averaging; what lies beside them keeps its fill; 2 frames"""
    import torch
    for w, h, s in [(18, 10, 420), (40, 24, 420), (18, 9, 422), (17, 9, 444), (2, 2, 420)]:
        cw, ch = (w if s == 444 else w // 2), (h // 2 if s == 420 else h)
        imgs = [lc.rgb_image(w, h, s, "noise"), lc.rgb_image(w, h, s, "gradient")]
        specs, po = [], 16
        for pw, ph in ((w, h), (cw, ch), (cw, ch)):
            stride = (pw + 7) // 8 * 8 + 8
            specs.append(dict(blocks_w=(pw + 7) // 8, blocks_h=(ph + 7) // 8, plane_offset=po, stride=stride))
            po += stride * ph + 24
        fs = (po + 7) // 8 * 8
        want = np.full((2, fs), FILL, dtype=np.uint8)
        for f, im in enumerate(imgs):
            for sp, p, (pw, ph) in zip(specs, ler.rgb_to_planes(im, s), ((w, h), (cw, ch), (cw, ch))):
                for y in range(ph):
                    want[f, sp["plane_offset"] + y * sp["stride"]:sp["plane_offset"] + y * sp["stride"] + pw] = p[y, :pw]
        rgb = np.stack(imgs) if layout == "interleaved" else np.ascontiguousarray(np.stack(imgs).transpose(0, 3, 1, 2))
        got = np.full((2, fs), FILL, dtype=np.uint8)
        if where == "host":
            ctx.rgb_to_yuv(rgb, w, h, s, got, specs, n_frames=2, yuv_frame_stride=fs, layout=layout)
        else:
            d_r, d_y = torch.from_numpy(rgb).cuda(), torch.from_numpy(got).cuda()
            ctx.rgb_to_yuv(d_r, w, h, s, d_y, specs, n_frames=2, yuv_frame_stride=fs, layout=layout)
            ctx.synchronize()
            got = d_y.cpu().numpy()
        assert np.array_equal(got, want), (w, h, s)


@pytest.fixture(scope="module")
def mixed_rgb_set(ctx):
    """(specs, images, hvc_jpeg_encode_rgb's file of each image alone under the setting; None for the odd-sized one in the middle)"""
    cases = [c for c in RGB_CASES if c[4] == "noise"]
    specs, images, alone = [], [], []
    for k, (name, w, h, s, kind, tab) in enumerate(cases):
        if k == len(cases) // 2:
            specs.append((17, 16, 420, 75))
            images.append(np.zeros((16, 17, 3), dtype=np.uint8))
            alone.append(None)
        images.append(lc.rgb_image(w, h, s, kind))
        specs.append((w, h, s, quality_of(tab)))
        alone.append(ctx.jpeg_encode_rgb(images[-1], s, quality_of(tab)))
    return specs, images, alone


@pytest.mark.parametrize("coder", ["host", "gpu"])
@pytest.mark.parametrize("chunk_bytes", [0, 4096], ids=["one_chunk", "small_chunks"])
def test_mixed_rgb_batch_equals_the_single_file_call(ctx, mixed_rgb_set, coder, chunk_bytes):
    specs, images, alone = mixed_rgb_set
    res = ctx.jpeg_encode_batch_mixed_rgb(images, specs, threads=2, chunk_bytes=chunk_bytes, coder=coder)
    assert [r[0] for r in res] == [0 if a is not None else E_INVALID_ARG for a in alone]
    assert [r[1] for r in res] == alone


# The smallest set with, in ONE launch of k_rgb_to_ycc_libjpeg_mixed, a last workgroup with spare units, a unit with a single
# active lane and an image with one lane per row (groups == 1): the single-block image, the 40 x 104 4:4:4 image (520 lanes: 9
# units) and two images of 65 lanes, 8 x 65 with one lane per row.  The lane grid is libjpeg_rgb_lane_grid's without padding
# (hvc_rgb_to_yuv_mixed): ceil(w / 8) x h here; under padding (hvc_encode_frames_mixed_rgb) a grid's height is a multiple of
# 8, so a unit of one lane cannot occur there -- that call has the spare units (1 + 9 + 2 + 2) and the one-lane rows.
EDGE_RGB = [("edge_rgb_%dx%d_%d" % c,) + c + ("noise", "q75") for c in ((8, 8, 444), (40, 104, 444), (8, 65, 422), (40, 13, 444))]


def test_the_edge_rgb_set_is_what_it_claims():
    lanes = [-(-w // 8) * h for _, w, h, s, _, _ in EDGE_RGB]
    padded = [-(-w // 8) * (-(-h // 8) * 8) for _, w, h, s, _, _ in EDGE_RGB]
    assert sum(-(-n // 64) for n in lanes) % 4 and sum(-(-n // 64) for n in padded) % 4
    assert sum(n % 64 == 1 for n in lanes) == 2 and any(w <= 8 and h > 64 for _, w, h, _, _, _ in EDGE_RGB)


@pytest.mark.parametrize("where", ["host", "device"])
def test_encode_frames_mixed_rgb_and_rgb_to_yuv_mixed(hvc, ctx, where):
    """records straight from RGB images of mixed geometry = the records of hvc_jpeg_encode_rgb's files; the planes of
    hvc_rgb_to_yuv_mixed = hvc_rgb_to_yuv's, the padding of the plane records untouched"""
    mixed_rgb_records_and_planes(hvc, ctx, where, [c for c in RGB_CASES if c[4] == "noise"], 0)


def test_mixed_rgb_spare_units_a_single_active_lane_and_one_lane_per_row(hvc, ctx):
    """EDGE_RGB in one launch, whole buffers over the fill with a guard region behind the last record"""
    mixed_rgb_records_and_planes(hvc, ctx, "device", EDGE_RGB, 4096)


def mixed_rgb_records_and_planes(hvc, ctx, where, cases, guard):
    import torch
    specs = [(w, h, s, quality_of(tab)) for _, w, h, s, _, tab in cases]
    lay = hvc.hvc.jpeg_encoder_mixed_rgb_layout(specs)
    assert not any(lay.status)
    rgb = np.full(lay.rgb_total, FILL, dtype=np.uint8)
    want = np.full(lay.coef_total + guard, FILL16, dtype=np.int16)
    planes_want = np.full(lay.pixel_total + guard, FILL, dtype=np.uint8)
    for f, case in enumerate(cases):
        name, w, h, s, kind, tab = case
        im = lc.rgb_image(w, h, s, kind)
        rs = lay.rgb_row_strides[f] or 3 * w
        for y in range(h):
            rgb[lay.rgb_offsets[f] + y * rs:lay.rgb_offsets[f] + y * rs + 3 * w] = im[y].reshape(-1)
        rec = rgb_reference(hvc, case)[0]
        want[lay.coef_offsets[f]:lay.coef_offsets[f] + rec.size] = rec
        for k, p in enumerate(ler.rgb_to_planes(im, s)):
            L = lay.infos[f].layout[k]
            aw, ah = lay.infos[f].comp[k].actual_width, lay.infos[f].comp[k].actual_height
            for y in range(ah):
                at = lay.pixel_offsets[f] + L.plane_offset + y * L.stride
                planes_want[at:at + aw] = p[y, :aw]
    got = np.full(lay.coef_total + guard, FILL16, dtype=np.int16)
    planes = np.full(lay.pixel_total + guard, FILL, dtype=np.uint8)
    if where == "host":
        ctx.encode_frames_mixed_rgb(rgb, lay.rgb_offsets, lay.infos, got, lay.coef_offsets, rgb_row_strides=lay.rgb_row_strides)
        ctx.rgb_to_yuv_mixed(planes, lay.pixel_offsets, lay.infos, rgb, lay.rgb_offsets, rgb_row_strides=lay.rgb_row_strides)
    else:
        d_r, d_c, d_p = torch.from_numpy(rgb).cuda(), torch.from_numpy(got).cuda(), torch.from_numpy(planes).cuda()
        ctx.encode_frames_mixed_rgb(d_r, lay.rgb_offsets, lay.infos, d_c, lay.coef_offsets, rgb_row_strides=lay.rgb_row_strides)
        ctx.rgb_to_yuv_mixed(d_p, lay.pixel_offsets, lay.infos, d_r, lay.rgb_offsets, rgb_row_strides=lay.rgb_row_strides)
        ctx.synchronize()
        got, planes = d_c.cpu().numpy(), d_p.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(planes, planes_want)
