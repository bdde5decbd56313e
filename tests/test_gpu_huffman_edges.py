"""The GPU table builder (k_huff_hist + k_huff_build of csrc/hvc_huff.hip, behind hvc_huffman_encode_frames_optimised and
its restart twin) on the record families of tests/huffman_records.py: trees that figure K.3 has to shorten, 16-bit codes
with 10 value bits, long runs of equal counts, the whole alphabet, tables of one symbol, a table without EOB; many
families in one call and a smaller call behind it on the same context; workgroups of k_huff_hist that walk several tiles
of different table sets (more than 1024 frames in a call, more than 2048); restart intervals.

Every comparison is exact equality of the four specs and of the segment's bytes.  The yardstick is the pure-Python Annex
K.2 writer (tools/jpeg_opt_writer.py); where a call has more frames than that writer covers in a few seconds, every frame
is held to the host composition hvc_huffman_optimal_tables + hvc_jpeg_entropy_encode_tables and a fixed sample to the
writer (tests/test_huffman_edge_records.py holds the host composition to the writer on the same families)."""
import numpy as np
import pytest

import huffman_records as R
from jpeg_opt_writer import jpeg_optimised_tables
from test_huffman_optimise import segments

pytestmark = pytest.mark.gpu

COMMON = (128, 88, 444)      # the geometry of the calls that mix families


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(hvc):
    c = hvc.Context(0)
    yield c
    c.close()


_records, _wanted = {}, {}


def family(hvc, name, w, h, chroma, check=True):
    """(info, record) of a family at a geometry, built once; check: with the family's property asserted"""
    key = (name, w, h, chroma)
    if key not in _records:
        info = hvc.hvc.jpeg_encoder_layout(w, h, chroma, R.QUALITY)
        if name.startswith("sparse"):
            rec = R.sparse_random(info, int(name[6:]))
        elif name == "chain17_reduced":      # chain17 in the blocks of the common geometry
            rec = R.chain17(info)
            assert R.max_code_size(R.symbol_counts(info, rec)[2]) >= 17
        else:
            rec = R.FAMILIES[name][0](info)
            if check:
                R.check_property(name, info, rec)
        rec.setflags(write=False)
        _records[key] = (info, rec)
    return _records[key]


def writer_wants(info, rec, w, h, chroma, ri=0):
    """(specs DC0 DC1 AC0 AC1, segment) of the Python writer's file"""
    jpg = jpeg_optimised_tables(w, h, chroma, info.qtab_array(), rec, table_sets=2, restart_interval=ri)
    dht, ecs = segments(jpg)
    return [(list(dht[(t >> 1, t & 1)][:16]), list(dht[(t >> 1, t & 1)][16:])) for t in range(4)], ecs


def wanted(hvc, name, w, h, chroma, ri=0, check=True):
    key = (name, w, h, chroma, ri)
    if key not in _wanted:
        info, rec = family(hvc, name, w, h, chroma, check)
        _wanted[key] = writer_wants(info, rec, w, h, chroma, ri)
    return _wanted[key]


def host_wants(hvc, info, rec):
    specs = hvc.hvc.huffman_optimal_tables(info, rec)
    jpg = hvc.hvc.jpeg_entropy_encode(info, rec, specs)
    return specs, jpg[len(hvc.hvc.jpeg_header(info, specs)):-2]


def on(device, a):
    if not device:
        return a
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared records are read-only)


def strided(recs, stride):
    out = np.zeros((len(recs), stride), dtype=np.int16)
    for f, r in enumerate(recs):
        out[f, :r.size] = r
    return out.reshape(-1)


# -- a: every family alone --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,w,h,chroma", R.CASES, ids=["%s-%dx%d-%d" % c for c in R.CASES])
def test_family_alone(ctx, hvc, name, w, h, chroma, device):
    info, rec = family(hvc, name, w, h, chroma)
    want_specs, want_seg = wanted(hvc, name, w, h, chroma)
    segs, specs = ctx.huffman_encode_frames_optimised(info, on(device, rec), info.coef_count, 1)
    assert specs[0] == want_specs
    assert segs[0] == want_seg


# -- b: every family in one call ----------------------------------------------------------------------------------------

MIXED = ["chain17_reduced", "ties", "whole_alphabet", "eob_only", "no_eob", "one_dc_category", "sparse5"]


def check_call(ctx, hvc, names, device):
    w, h, chroma = COMMON
    info = family(hvc, names[0], w, h, chroma, check=False)[0]
    stride = (info.coef_count + 7) // 8 * 8 + 8       # records not back to back
    coefs = on(device, strided([family(hvc, nm, w, h, chroma, check=False)[1] for nm in names], stride))
    segs, specs = ctx.huffman_encode_frames_optimised(info, coefs, stride, len(names))
    for f, nm in enumerate(names):
        want_specs, want_seg = wanted(hvc, nm, w, h, chroma, check=False)
        assert specs[f] == want_specs, "frame %d (%s)" % (f, nm)
        assert segs[f] == want_seg, "frame %d (%s)" % (f, nm)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", [7, 64])
def test_families_in_one_call_then_fewer_frames(ctx, hvc, n, device):
    """frames cycle through the families at one geometry (ties and whole_alphabet as near their property as 176 blocks
    allow): every frame's tables and segment are its own, and so are those of a call of 3 frames in another order behind
    it -- counts, tables or specs left over from the larger call would show"""
    assert R.max_code_size(R.symbol_counts(*family(hvc, "chain17_reduced", *COMMON))[2]) >= 17
    check_call(ctx, hvc, [MIXED[f % len(MIXED)] for f in range(n)], device)
    check_call(ctx, hvc, ["eob_only", "chain17_reduced", "no_eob"], device)
    check_call(ctx, hvc, ["whole_alphabet"], device)


# -- c: the tile loop of k_huff_hist ------------------------------------------------------------------------------------

POOL, SAMPLE = 127, 40       # distinct records per geometry; how many of them the Python writer covers


def pool(hvc, w, h):
    """POOL records of a 4:2:0 geometry -- seeded sparse random ones of several densities, every 16th eob_only, every 16th
    no_eob -- with the host composition's specs and segment for each, the first SAMPLE of them held to the Python writer"""
    key = ("pool", w, h)
    if key not in _records:
        info = hvc.hvc.jpeg_encoder_layout(w, h, 420, R.QUALITY)
        recs, wants = [], []
        for i in range(POOL):
            if i % 16 == 3:
                rec = R.eob_only(info)
            elif i % 16 == 7:
                rec = R.no_eob(info, seed=900 + i)
            else:
                rec = R.sparse_random(info, 500 + i, density=(0.03, 0.15, 0.6)[i % 3], cmax=(3, 60, 1023)[(i // 3) % 3])
            want = host_wants(hvc, info, rec)
            if i < SAMPLE:
                assert want == writer_wants(info, rec, w, h, 420), "pool record %d" % i
            recs.append(rec)
            wants.append(want)
        _records[key] = (info, recs, wants)
    return _records[key]


@pytest.mark.parametrize("n", [1000, 2049, 4100])
@pytest.mark.parametrize("w,h", [(16, 16), (48, 32)])
def test_workgroups_walk_tiles_of_both_table_sets(ctx, hvc, w, h, n):
    """3 tiles a frame (Y, U, V) and 2, 1 and 1 workgroups for them: a workgroup counts a luma and a chroma tile, into
    different table sets; every frame is held to the host composition (frame f is pool record 31 f mod 127, so the
    neighbours differ)"""
    info, recs, wants = pool(hvc, w, h)
    which = [(31 * f) % POOL for f in range(n)]
    assert set(range(SAMPLE)) <= set(which)
    coefs = np.stack([recs[i] for i in which]).reshape(-1)
    segs, specs = ctx.huffman_encode_frames_optimised(info, coefs, info.coef_count, n)
    bad = [f for f in range(n) if specs[f] != wants[which[f]][0] or segs[f] != wants[which[f]][1]]
    assert not bad, "%d frames differ, the first: %s" % (len(bad), bad[:8])


def test_chain20_alone_and_among_1000_frames(ctx, hvc):
    """a 4:2:0 chain20 frame (8 + 2 + 2 tiles) alone, one workgroup per tile, and as frame 617 of 1000, where two
    workgroups walk its twelve tiles"""
    w, h, chroma = 512, 256, 420
    info, rec = family(hvc, "chain20", w, h, chroma)
    want_specs, want_seg = wanted(hvc, "chain20", w, h, chroma)
    segs, specs = ctx.huffman_encode_frames_optimised(info, rec, info.coef_count, 1)
    assert (specs[0], segs[0]) == (want_specs, want_seg)
    n, at = 1000, 617
    others = [R.sparse_random(info, 40 + i, density=0.02, cmax=7) for i in range(3)]
    others.append(R.eob_only(info))
    other_wants = [host_wants(hvc, info, r) for r in others]
    coefs = np.empty((n, info.coef_count), dtype=np.int16)
    for i, r in enumerate(others):
        coefs[i::len(others)] = r
    coefs[at] = rec
    segs, specs = ctx.huffman_encode_frames_optimised(info, coefs.reshape(-1), info.coef_count, n)
    assert (specs[at], segs[at]) == (want_specs, want_seg)
    bad = [f for f in range(n) if f != at and (specs[f], segs[f]) != other_wants[f % len(others)]]
    assert not bad, "%d frames differ, the first: %s" % (len(bad), bad[:8])


# -- d: restart intervals -------------------------------------------------------------------------------------------------

RESTART_CASES = [c for c in R.CASES if c[0] in ("chain20", "eob_only", "one_dc_category")]


@pytest.mark.parametrize("name,w,h,chroma", RESTART_CASES, ids=["%s-%dx%d-%d" % c for c in RESTART_CASES])
def test_family_with_restart_intervals(ctx, hvc, name, w, h, chroma):
    """k_huff_hist_rst with the predictor chain cut every 1 and 5 MCUs; an interval of the whole scan is the plain result"""
    info, rec = family(hvc, name, w, h, chroma)
    n_mcu = np.prod(R.mcu_grid(info))
    for ri in (1, 5):
        want_specs, want_seg = wanted(hvc, name, w, h, chroma, ri)
        segs, specs = ctx.huffman_encode_frames_optimised(info, rec, info.coef_count, 1, restart_interval=ri)
        assert specs[0] == want_specs, ri
        assert segs[0] == want_seg, ri
    want_specs, want_seg = wanted(hvc, name, w, h, chroma)
    for ri in (int(n_mcu), int(n_mcu) + 3):
        segs, specs = ctx.huffman_encode_frames_optimised(info, rec, info.coef_count, 1, restart_interval=ri)
        assert (specs[0], segs[0]) == (want_specs, want_seg), ri


def test_unused_table_set_is_refused_as_on_the_host(ctx, hvc):
    """all three components on one table set -- an info hvc_jpeg_encoder_check lets through -- leave the other set without
    a symbol to fit a table to: HVC_E_INVALID_ARG, hvc_huffman_optimal_tables' answer, before anything is launched"""
    import ctypes as C
    info = hvc.hvc.jpeg_encoder_layout(64, 48, 444, R.QUALITY)
    rec = R.sparse_random(info, 3)
    for sel in (0, 1):
        one = hvc.hvc.JpegInfo.from_buffer_copy(info)
        for i in range(3):
            one.comp[i].dc_table = one.comp[i].ac_table = sel
        assert hvc.lib().hvc_jpeg_encoder_check(C.byref(one)) == 0
        out = (hvc.hvc.HuffSpec * 4)()
        assert hvc.lib().hvc_huffman_optimal_tables(C.byref(one), rec.ctypes.data, out) == -1
        for ri in (0, 2):
            with pytest.raises(hvc.hvc.HvcError) as e:
                ctx.huffman_encode_frames_optimised(one, rec, info.coef_count, 1, restart_interval=ri)
            assert e.value.code == -1
    # the context codes the next frame as before
    segs, specs = ctx.huffman_encode_frames_optimised(info, rec, info.coef_count, 1)
    assert (specs[0], segs[0]) == host_wants(hvc, info, rec)


# -- f: the default tables afterwards -----------------------------------------------------------------------------------

def test_default_tables_after_optimised(ctx, hvc):
    w, h, chroma = 256, 192, 444
    info, rec = family(hvc, "chain20", w, h, chroma)
    ctx.huffman_encode_frames_optimised(info, rec, info.coef_count, 1)
    jpg = hvc.hvc.jpeg_entropy_encode(info, rec)
    assert ctx.huffman_encode_frames(info, rec, info.coef_count, 1)[0] == jpg[len(hvc.hvc.jpeg_header(info)):-2]


# -- e: back through the readers ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,w,h,chroma", R.CASES, ids=["%s-%dx%d-%d" % c for c in R.CASES])
def test_files_read_back_to_the_record(ctx, hvc, name, w, h, chroma):
    """header + the GPU's segment + EOI through the GPU reader and the host reader (which of the two the GPU entry point
    used is not asserted: a table of many long codes may rightly go to the host reader)"""
    info, rec = family(hvc, name, w, h, chroma)
    segs, specs = ctx.huffman_encode_frames_optimised(info, rec, info.coef_count, 1)
    jpg = hvc.hvc.jpeg_header(info, specs[0]) + segs[0] + b"\xff\xd9"
    _, got = hvc.hvc.jpeg_entropy_decode(jpg)
    assert np.array_equal(got.reshape(-1)[:rec.size], rec)
    for device in (False, True):
        _, got, _ = ctx.jpeg_entropy_decode_gpu([jpg], device=device)
        assert np.array_equal(got[0].reshape(-1)[:rec.size], rec)
