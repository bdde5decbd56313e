"""The mixed GPU Huffman coder alone (hvc_huffman_encode_frames_mixed, csrc/hvc_huff_mixed.hip): coefficient records of
frames of different geometry coded in one chain of launches, against the HOST coder frame by frame -- hvc_jpeg_entropy_encode /
hvc_jpeg_entropy_encode_tables with the header and EOI stripped -- exactly."""
import ctypes as C

import numpy as np
import pytest

from huffman_records import blocks_of, symbol_counts

pytestmark = pytest.mark.gpu

E_INVALID_ARG, E_ALIGNMENT, E_RANGE = -1, -4, -5
FILL = 0xA5

# (width, height, chroma, quality): three planes of one block; one MCU of six blocks; planes larger than the MCU grid (4:2:0
# and 4:2:2); planes of 64 / 16 / 16 blocks; 72 blocks (a unit boundary); bw = 1 and 257 blocks (a workgroup boundary); more
# than 4096 coded blocks (a second round of the per-file scan).  Quality 100: noise frames, whose segments hold 0xFF bytes.
GEOMS = [(8, 8, 444, 100), (2, 2, 420, 100), (24, 24, 420, 75), (40, 24, 422, 100), (64, 64, 420, 50), (72, 64, 444, 100),
         (8, 2056, 444, 100), (520, 264, 422, 100)]


@pytest.fixture()
def ctx():
    import video_coding_amd as hvc
    c = hvc.Context(0)
    yield c
    c.close()


def host_segment(info, rec, optimised):
    """(scan data of the host coder's file, its tables or None); an hvc_status where the host coder refuses the record"""
    import video_coding_amd as hvc
    try:
        if optimised:
            specs = hvc.hvc.huffman_optimal_tables(info, rec)
            jpg, head = hvc.hvc.jpeg_entropy_encode(info, rec, specs), hvc.hvc.jpeg_header(info, specs)
        else:
            specs = None
            jpg, head = hvc.hvc.jpeg_entropy_encode(info, rec), hvc.hvc.jpeg_header(info)
    except hvc.HvcError as e:
        return e.code, None
    assert jpg[:len(head)] == head and jpg[-2:] == b"\xff\xd9"
    return jpg[len(head):-2], specs


def hand_made(hvc):
    """[(name, info, record)] on 16 x 16 4:4:4 (three planes of four blocks) and 8 x 8 4:4:4"""
    info = hvc.hvc.jpeg_encoder_layout(16, 16, 444, 75)
    small = hvc.hvc.jpeg_encoder_layout(8, 8, 444, 75)
    out = []
    zero = lambda i=info: np.zeros(i.coef_count, dtype=np.int16)
    out.append(("zeros", info, zero()))                    # EOB only: a segment of a few bytes, 56 bits
    out.append(("zeros_8x8", small, zero(small)))          # ... and 14 bits
    r = zero()
    r.reshape(-1, 64)[:, 63] = np.where(np.arange(12) & 1, 5, -3)   # a non-zero last coefficient: no EOB
    out.append(("no_eob", info, r))
    r = zero()
    for b, k in enumerate((16, 17, 33, 49) * 3):           # zero runs of 15, 16, 32 and 48 in front of a value: ZRL
        r.reshape(-1, 64)[b, k] = (b % 5 + 1) * (-1 if b & 1 else 1)
    out.append(("zrl", info, r))
    r = zero()
    blk = r.reshape(-1, 64)
    blk[:, 0] = np.where(np.arange(12) & 1, -1024, 1023)   # DC differences of +-2047 along every component's scan
    blk[:, 1], blk[:, 40], blk[:, 63] = 1023, -1023, 1023  # the largest AC codes
    out.append(("largest", info, r))
    return out


def flagged(hvc):
    info = hvc.hvc.jpeg_encoder_layout(16, 16, 444, 75)
    dc = np.zeros(info.coef_count, dtype=np.int16)
    b = blocks_of(info, dc, 1)
    b[:, 0] = np.where(np.arange(len(b)) & 1, -1024, 1024)  # a DC difference of 2048: category 12
    b[:, 5] = 9
    ac = np.zeros(info.coef_count, dtype=np.int16)
    blocks_of(info, ac, 0)[2, 30] = 1024                    # an AC value of size 11
    blocks_of(info, ac, 2)[:, 1] = -4
    return [("dc2048", info, dc), ("ac1024", info, ac)]


@pytest.fixture(scope="module")
def records():
    """[(name, info, record)]: the geometries' records from hvc_encode_frames_mixed on seeded frames with structure and noise,
    then the hand-made ones; with the host coder's segment of each under both table modes (computed once, never changed)"""
    import video_coding_amd as hvc
    lay = hvc.hvc.jpeg_encoder_mixed_layout(GEOMS)
    assert list(lay.status[:len(GEOMS)]) == [0] * len(GEOMS)
    pixels = np.zeros(lay.pixel_total + 8, dtype=np.uint8)
    for k in range(len(GEOMS)):
        rng = np.random.Generator(np.random.PCG64(4200 + k))
        info = lay.infos[k]
        for i in range(3):
            pw, ph, L = info.comp[i].decoded_width, info.comp[i].decoded_height, info.layout[i]
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = np.clip(128 + 90 * np.sin(xx / 5.0 + k) * np.cos(yy / 7.0) + rng.integers(-40, 41, size=(ph, pw)), 0, 255).astype(np.uint8)
            at = lay.pixel_offsets[k] + L.plane_offset
            view = pixels[at:at + (ph - 1) * L.stride + pw]
            for row in range(ph):
                view[row * L.stride:row * L.stride + pw] = p[row]
    coefs = np.zeros(lay.coef_total, dtype=np.int16)
    c = hvc.Context(0)
    c.encode_frames_mixed(pixels, list(lay.pixel_offsets)[:len(GEOMS)], lay.infos, coefs, list(lay.coef_offsets)[:len(GEOMS)])
    c.close()
    out = [("%dx%d_%d" % g[:3], hvc.hvc.JpegInfo.from_buffer_copy(bytes(lay.infos[k])),
            coefs[lay.coef_offsets[k]:lay.coef_offsets[k] + lay.infos[k].coef_count].copy()) for k, g in enumerate(GEOMS)]
    out += hand_made(hvc)
    want = {opt: [host_segment(info, rec, opt) for _, info, rec in out] for opt in (False, True)}
    return out, want


def place(recs, device, gap=24):
    """the records `gap` elements apart (each on 16 bytes) -> (coefs, offsets)"""
    offs, at = [], 8
    for _, info, _ in recs:
        offs.append(at)
        at += (info.coef_count + gap + 7) // 8 * 8
    buf = np.full(at, 0x5A5A, dtype=np.int16)
    for (_, _, rec), o in zip(recs, offs):
        buf[o:o + rec.size] = rec
    if device:
        import torch
        buf = torch.from_numpy(buf).cuda()
    return buf, offs


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("optimised", [False, True], ids=["default", "optimised"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_segments_equal_the_host_coders(ctx, records, device, optimised, reverse):
    recs, want = records
    order = list(range(len(recs)))[::-1] if reverse else list(range(len(recs)))
    recs = [recs[k] for k in order]
    want = [want[optimised][k] for k in order]
    coefs, offs = place(recs, device)
    segs, status, specs = ctx.huffman_encode_frames_mixed([r[1] for r in recs], coefs, offs, optimised=optimised)
    assert status == [0] * len(recs)
    for k, (name, _, _) in enumerate(recs):
        assert segs[k] == want[k][0], name
        if optimised:
            assert specs[k] == want[k][1], name                  # == hvc_huffman_optimal_tables
    assert min(len(s) for s in segs) < 16 < 4096 < max(len(s) for s in segs)


def test_hand_made_records_are_what_they_claim(records):
    """EOB only / no EOB / ZRL / the largest codes, by the Python counter; a bit total that is a multiple of 8 and one that
    is not, from the default tables' code lengths"""
    import video_coding_amd as hvc
    recs, want = records
    by_name = {name: (info, rec) for name, info, rec in recs}
    tabs = []
    for t in range(2):
        codes = np.zeros(16 + 256, dtype=np.uint32)
        assert hvc.lib().hvc_huffman_code_tables(None, t, 0, codes.ctypes.data) == 0
        tabs.append(codes & 31)

    def bits(name):
        info, rec = by_name[name]
        dc0, dc1, ac0, ac1 = symbol_counts(info, rec)
        return sum(n * (int(tabs[t][s]) + s) for t, dc in enumerate((dc0, dc1)) for s, n in enumerate(dc) if n) + \
            sum(n * (int(tabs[t][16 + s]) + (s & 15)) for t, ac in enumerate((ac0, ac1)) for s, n in enumerate(ac) if n)

    assert bits("zeros") == 56 and bits("zeros_8x8") == 14      # a multiple of 8, and not
    assert len(want[False][[r[0] for r in recs].index("zeros")][0]) == 7   # a segment of a few bytes
    _, _, ac0, ac1 = symbol_counts(*by_name["zeros"])
    assert [s for s in range(256) if ac0[s]] == [0] and [s for s in range(256) if ac1[s]] == [0]
    _, _, ac0, ac1 = symbol_counts(*by_name["no_eob"])
    assert ac0[0] == ac1[0] == 0 and ac0[0xF0] == 3 * 4
    _, _, ac0, ac1 = symbol_counts(*by_name["zrl"])
    assert ac0[0xF0] == 0 + 1 + 2 + 3 and ac1[0xF0] == 2 * (0 + 1 + 2 + 3)    # runs of 15, 16, 32 and 48 in every plane
    assert sum(ac0[0xF0 | s] for s in range(1, 11)) == 1                      # ... the run of 15 without a ZRL
    dc0, dc1, ac0, ac1 = symbol_counts(*by_name["largest"])
    assert dc0[11] == 3 and dc1[11] == 6 and ac0[0x0A] == 4 and ac1[0x0A] == 8   # differences of +-2047, AC of +-1023


def test_stuffing_reaches_past_the_first_piece(records):
    """the noise frames' expected segments hold FF 00, at least once in a 64-byte piece of the unstuffed segment that is not
    the first"""
    recs, want = records
    for k, g in enumerate(GEOMS):
        if g[3] != 100 or g[0] * g[1] < 72 * 64:
            continue
        seg = np.frombuffer(want[False][k][0], dtype=np.uint8)
        at = np.flatnonzero((seg[:-1] == 0xFF) & (seg[1:] == 0))
        assert len(at), recs[k][0]
        unstuffed = at - np.arange(len(at))                      # where the 0xFF stands before stuffing
        assert (unstuffed >= 64).any(), recs[k][0]


@pytest.mark.parametrize("optimised", [False, True], ids=["default", "optimised"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_flagged_file_is_empty_and_its_neighbours_are_right(ctx, records, device, optimised):
    import video_coding_amd as hvc
    recs, want = records
    bad = flagged(hvc)
    for _, info, rec in bad:
        assert host_segment(info, rec, False)[0] == E_RANGE      # the host coder refuses them too
    pick = [2, 8, 12]                                            # 24x24 4:2:0, zeros, largest
    mixed = [recs[pick[0]], bad[0], recs[pick[1]], bad[1], recs[pick[2]]]
    coefs, offs = place(mixed, device)
    segs, status, specs = ctx.huffman_encode_frames_mixed([r[1] for r in mixed], coefs, offs, optimised=optimised)
    assert status == [0, E_RANGE, 0, E_RANGE, 0]
    assert segs[1] == b"" and segs[3] == b""
    for k, p in ((0, pick[0]), (2, pick[1]), (4, pick[2])):
        assert segs[k] == want[optimised][p][0], k
        if optimised:
            assert specs[k] == want[True][p][1]
    if optimised:
        assert specs[1] is None and specs[3] is None


def test_four_small_files_get_four_table_sets(ctx):
    """four files of one unit per plane and different content, their units side by side in the same workgroups: each file's
    own tables, equal to hvc_huffman_optimal_tables'"""
    import video_coding_amd as hvc
    info = hvc.hvc.jpeg_encoder_layout(16, 16, 444, 75)
    recs = []
    for k in range(4):
        rng = np.random.default_rng(70 + k)
        r = np.zeros(info.coef_count, dtype=np.int16)
        b = r.reshape(-1, 64)
        b[:, 0] = rng.integers(-(20 << k), (20 << k) + 1, size=12)
        b[:, 1 + k:9 + 3 * k] = rng.integers(-(2 << k), (2 << k) + 1, size=(12, 8 + 2 * k))
        recs.append(("small%d" % k, info, r))
    coefs, offs = place(recs, False)
    segs, status, specs = ctx.huffman_encode_frames_mixed([info] * 4, coefs, offs, optimised=True)
    assert status == [0] * 4
    want = [host_segment(info, r, True) for _, _, r in recs]
    for k in range(4):
        assert specs[k] == want[k][1] and segs[k] == want[k][0], k
    assert len({repr(s) for s in specs}) == 4


def test_capacity_fill_bytes_and_an_empty_set(ctx, records):
    import torch
    import video_coding_amd as hvc
    recs, want = records
    part = recs[:6]
    total = sum(len(want[False][k][0]) for k in range(6))
    for device in (False, True):
        coefs, offs = place(part, device)
        make = (lambda n: torch.full((n,), FILL, dtype=torch.uint8, device="cuda")) if device else (lambda n: np.full(n, FILL, dtype=np.uint8))
        host = (lambda t: t.cpu().numpy()) if device else (lambda t: t)
        out = make(total + 100)
        with pytest.raises(hvc.HvcError) as e:                    # one byte short: nothing is written
            ctx.huffman_encode_frames_mixed([r[1] for r in part], coefs, offs, out_cap=total - 1, out=out)
        assert e.value.code == E_INVALID_ARG and (host(out) == FILL).all()
        segs, status, _ = ctx.huffman_encode_frames_mixed([r[1] for r in part], coefs, offs, out_cap=total, out=out)
        assert status == [0] * 6 and b"".join(segs) == b"".join(want[False][k][0] for k in range(6))
        got = host(out)
        assert got[:total].tobytes() == b"".join(segs) and (got[total:] == FILL).all()   # nothing behind the segments is written
        untouched = host(coefs)
        assert (untouched[:offs[0]] == 0x5A5A).all()
    # an empty set needs no memory and launches nothing
    segs, status, specs = ctx.huffman_encode_frames_mixed([], None, [])
    assert (segs, status, specs) == ([], [], None)
    assert hvc.lib().hvc_huffman_encode_frames_mixed(ctx._h, None, None, None, 0, 1, None, 0, None, None, None, 1) == 0


def test_refusals_of_the_call(ctx, records):
    import torch
    import video_coding_amd as hvc
    recs, _ = records
    name, info, rec = recs[2]
    L = hvc.lib().hvc_huffman_encode_frames_mixed
    infos = (hvc.hvc.JpegInfo * 1)(info)
    buf = np.zeros(rec.size + 16, dtype=np.int16)
    out = np.full(4096, FILL, dtype=np.uint8)
    offs, status = np.zeros(2, dtype=np.uint64), (C.c_int * 1)(77)
    specs = (hvc.hvc.HuffSpec * 4)()
    co = lambda v: (C.c_size_t * 1)(v)
    args = lambda **kw: [kw.get(k, d) for k, d in (("ctx", ctx._h), ("infos", infos), ("coefs", buf.ctypes.data), ("co", co(0)), ("n", 1),
                                                   ("tables", 0), ("out", out.ctypes.data), ("cap", out.size), ("offs", offs.ctypes.data),
                                                   ("status", status), ("specs", None), ("where", 0))]
    assert L(*args()) == 0
    for bad in (dict(ctx=None), dict(infos=None), dict(coefs=None), dict(co=None), dict(n=-1), dict(tables=2), dict(out=None),
                dict(offs=None), dict(status=None), dict(where=2), dict(tables=1)):          # (optimised without specs)
        assert L(*args(**bad)) == E_INVALID_ARG, bad
    assert L(*args(tables=1, specs=specs)) == 0
    assert L(*args(co=co(4))) == E_ALIGNMENT                      # a record off 16 bytes
    d = torch.zeros(rec.size + 16, dtype=torch.int16, device="cuda")
    d_out, d_offs = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L(*args(coefs=d.data_ptr() + 2, out=d_out.data_ptr(), offs=d_offs.data_ptr(), where=1)) == E_ALIGNMENT
    assert L(*args(coefs=d.data_ptr(), out=d_out.data_ptr(), offs=d_offs.data_ptr() + 4, where=1)) == E_ALIGNMENT
    assert L(*args(coefs=d.data_ptr(), out=d_out.data_ptr(), offs=d_offs.data_ptr(), where=1)) == 0
    # a frame the plan refuses has its own code and stops nobody
    refused = hvc.hvc.jpeg_encoder_layout(33, 16, 420, 75)
    both = [refused, info]
    coefs, o = place([("refused", refused, np.zeros(refused.coef_count, np.int16)), recs[2]], False)
    segs, st, _ = ctx.huffman_encode_frames_mixed(both, coefs, o)
    assert st == [E_INVALID_ARG, 0] and segs[0] == b"" and segs[1] == host_segment(info, rec, False)[0]
